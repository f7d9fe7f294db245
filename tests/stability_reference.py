"""Damping, the angular speed cap and the contact correction scalars restated in float64 on top of tests/lcp_dense.py and
tests/joint_dense.py, from the definitions in include/dmx_batch.h ("damping").

Test infrastructure, not a test file, and no code of the product.  lcp_dense and joint_dense stay as they are: their Island is
subclassed, the normal rows' c and with it b are recomputed from the definition

    depth = max(depth - surface_layer, 0);  c = erp * depth / h;  c = min(c, max_correcting_vel);  then the bounce rule

and `step` is restated with the damping in front

    if lin_scale != 0 and lvel.lvel > lin_threshold^2:  lvel *= (1 - lin_scale)        (ALIVE, not KINEMATIC, stepped)
    if ang_scale != 0 and avel.avel > ang_threshold^2:  avel *= (1 - ang_scale)

and the cap between the velocities and the poses

    if avel.avel > max^2:  avel *= max / sqrt(avel.avel)                                (not KINEMATIC)

The threshold is the feature's only discontinuity.  `step` reports, per stepped body whose scale is not zero, the relative
distance of lvel.lvel and avel.avel from their squared thresholds; `margin_ok` is the condition under which a float32 device and
this float64 reference may be compared: every such distance is at least MARGIN.
"""
import numpy as np

import autodisable_reference as ar
import joint_dense as jd
import lcp_dense as ld

MARGIN = 1e-3                                        # a condition on the scenes, never a tolerance
DEFAULT_ENTRY = (0.0, 0.0, 0.01, 0.01, np.inf)       # lin_scale, ang_scale, lin_threshold, ang_threshold, max_angular_speed
LIN_SCALE, ANG_SCALE, LIN_THRESHOLD, ANG_THRESHOLD, MAX_ANG_SPEED = range(5)


class Knobs:
    """the per-slot table (n, 5) and the batch's two contact scalars; the defaults are ODE's, all no-ops"""

    def __init__(self, n, table=None, surface_layer=0.0, max_correcting_vel=np.inf):
        self.table = np.tile(np.array(DEFAULT_ENTRY), (n, 1)) if table is None else np.array(table, np.float64).reshape(n, 5)
        self.surface_layer, self.max_correcting_vel = float(surface_layer), float(max_correcting_vel)

    def set_damping(self, lin_scale, ang_scale, lin_threshold=0.01, ang_threshold=0.01):
        self.table[:, :4] = (lin_scale, ang_scale, lin_threshold, ang_threshold)
        return self

    def set_max_angular_speed(self, v):
        self.table[:, MAX_ANG_SPEED] = v
        return self

    def as_precision(self, prec):
        """the values as a batch of this precision holds them"""
        if np.dtype(prec).itemsize == 8:
            return self
        r = lambda x: np.asarray(x, np.float32).astype(np.float64)
        return Knobs(len(self.table), r(self.table), float(r(self.surface_layer)), float(r(self.max_correcting_vel)))

    def is_default(self):
        return bool(np.all(self.table == np.array(DEFAULT_ENTRY))) and self.surface_layer == 0.0 and self.max_correcting_vel == np.inf


def _correct_normal_rows(I, world, jts, knobs):
    """recompute c of every contact's normal row with the two scalars, then b.  The rows' J and the island's v are the base
    class's; with the defaults every operation is the base class's own, in its order"""
    h = I.h
    for i in range(I.m):
        if I.row_kind[i] != 0:
            continue
        j = jts[I.row_joint[i]]
        mode = int(j["mode"])
        erp = float(j["soft_erp"]) if mode & ld.CONTACT_SOFT_ERP else world.erp
        cval = erp * max(float(j["depth"]) - knobs.surface_layer, 0.0) / h
        cval = min(cval, knobs.max_correcting_vel)
        if mode & ld.CONTACT_BOUNCE:
            outgoing = I.J[i] @ I.v
            if j["bounce_vel"] >= 0 and -outgoing > j["bounce_vel"]:
                cval = max(cval, -float(j["bounce"]) * outgoing)
        I.c[i] = cval
    I.b = I.c / h - I.J @ (I.v / h + I.minv(I.f))


class Island(ld.Island):
    """lcp_dense's island with the contact correction scalars in its normal rows"""

    def __init__(self, bodies, world, slots, cj, jts, knobs):
        super().__init__(bodies, world, slots, cj, jts)
        _correct_normal_rows(self, world, jts, knobs)


class JointIsland(jd.Island):
    """joint_dense's island (articulation rows ahead of the contacts', untouched) with the same"""

    def __init__(self, bodies, world, slots, members, jts, art, knobs):
        super().__init__(bodies, world, slots, members, jts, art)
        _correct_normal_rows(self, world, jts, knobs)


def damp(bodies, knobs, stepped=None):
    """the start-of-tick rule -> (damped copy of bodies, list of relative distances from the squared thresholds)"""
    out = bodies.copy()
    rel = []
    for s in (range(bodies.n) if stepped is None else stepped):
        if (int(bodies.flags[s]) & (ld.ALIVE | ld.KINEMATIC)) != ld.ALIVE:
            continue
        d = knobs.table[s]
        for vel, scale, thr in ((out.lvel, d[LIN_SCALE], d[LIN_THRESHOLD]), (out.avel, d[ANG_SCALE], d[ANG_THRESHOLD])):
            if scale == 0:
                continue
            vv, t2 = float(vel[s] @ vel[s]), thr * thr
            rel.append(abs(vv - t2) / t2 if t2 > 0 else (np.inf if vv > 0 else 0.0))
            if vv > t2:
                vel[s] = vel[s] * (1.0 - scale)
    return out, rel


def cap(avel, max_speed):
    ww = float(avel @ avel)
    if ww > max_speed * max_speed:
        return avel * (max_speed / np.sqrt(ww))
    return avel


def step(bodies, world, jts, stepper="quick", knobs=None, art=None):
    """one dmxBatchStepJoints tick with the four knobs -> lcp_dense.Result, which also carries `.damped` (the Bodies the rows were
    built from) and `.threshold_distance` (see the module's docstring).  `bodies` is not changed."""
    knobs = Knobs(bodies.n) if knobs is None else knobs
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    have_art = art is not None and len(art) > 0
    members = (jd.canonical_arts(bodies, art) if have_art else []) + ld.canonical(bodies, jts)
    damped, rel = damp(bodies, knobs)
    out = damped.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, ms in ld.islands(damped, members):
        I = JointIsland(damped, world, slots, ms, jts, art, knobs) if have_art else Island(damped, world, slots, ms, jts, knobs)
        if stepper == "quick":
            lam, margin = I.quickstep(world.iters, world.sor_w)
            info = {}
        else:
            lam, info = I.exact()
            margin = None
        v = I.velocities(lam)
        for k, s in enumerate(slots):
            if damped.flags[s] & ld.KINEMATIC:
                lv, av = damped.lvel[s], damped.avel[s]
            else:
                lv, av = v[6 * k:6 * k + 3], cap(v[6 * k + 3:6 * k + 6], knobs.table[s, MAX_ANG_SPEED])
            out.lvel[s], out.avel[s] = lv, av
            out.pos[s] = damped.pos[s] + h * lv
            q = damped.quat[s] + 0.5 * h * ld.quat_mul(np.concatenate([[0.0], av]), damped.quat[s])
            out.quat[s] = q / np.linalg.norm(q)
        isl.append(I)
        lams.append(lam)
        infos.append(info)
        margins.append(margin)
    r = ld.Result(out, isl, lams, infos, margins)
    r.damped, r.threshold_distance = damped, rel
    return r


def margin_ok(result):
    """no stepped body with a scale is within MARGIN (relative) of its squared threshold"""
    return all(d >= MARGIN for d in result.threshold_distance)


def step_autodisable(bodies, world, jts, stepper, knobs, params, counters):
    """autodisable_reference.step driven with the damped tick: asleep islands are left out whole (not damped either), the
    end-of-tick rule sees the post-step velocities -> autodisable_reference.Tick"""
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    awake, asleep = ar.split_islands(bodies, jts)
    awake_slots = sorted(s for slots, _ in awake for s in slots)
    asleep_slots = sorted(s for slots, _ in asleep for s in slots)
    t = ar.Tick()
    t.woken = [s for s in awake_slots if bodies.flags[s] & ar.DISABLED]
    t.skipped_islands, t.asleep_before, t.stepped = len(asleep), asleep_slots, awake_slots
    keep = np.zeros(len(jts), bool)
    for _, idx in awake:
        keep[idx] = True
    work = bodies.copy()
    work.flags[t.woken] &= np.uint8(~ar.DISABLED & 0xff)
    flags = work.flags.copy()
    work.flags[asleep_slots] &= np.uint8(~ld.ALIVE & 0xff)
    t.result = step(work, world, jts[keep], stepper, knobs)
    out = t.result.bodies
    out.flags = flags
    t.pre_lvel, t.pre_avel = out.lvel.copy(), out.avel.copy()
    cnt = counters.copy()
    t.slept = []
    for s in awake_slots:
        lv, av, f, st, tl = ar.idle_rule(out.lvel[s], out.avel[s], int(flags[s]), cnt.steps[s], cnt.time[s], params, world.h)
        if (f & ar.DISABLED) and not (flags[s] & ar.DISABLED):
            t.slept.append(s)
        out.lvel[s], out.avel[s], out.flags[s], cnt.steps[s], cnt.time[s] = lv, av, f, st, tl
    t.bodies, t.counters, t.contacts = out, cnt, int(keep.sum())
    return t
