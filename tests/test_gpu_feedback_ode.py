"""The ODE face of feedback (include/ode/ode.h: dJointSetFeedback / dJointGetFeedback), through ctypes on both ODE libraries (dReal =
double and dReal = float) as tests/test_gpu_slider_ode.py loads them: a ball, a hinge with a motor, a slider at a stop attached as
(0, body), a fixed joint, and the contact joints a near callback makes between a box and the ground plane.  The structs the steps
fill are compared with tests/feedback_dense.py from the poses the library reported before the step, by test_gpu_feedback.py's rule
(the same function), under both steppers; and a world none of whose joints has a struct is shown to take the same path -- the
single-launch tick -- with and without structs set elsewhere, from the batch's own report in a process of its own.

The scenes of tests/test_gpu_feedback.py's cases 1 to 3 run through the same calls (Built): bodies from dBodyCreate / dBodySetMass,
joints from dJointCreate* at the scene's sides, axes, stops and motors, the scene's contact joints from dJointCreateContact, a
struct on every one of them.  One thing cannot be carried over: ODE's sliders and fixed joints have no anchor of the caller's
choosing -- dJointSetSliderAxis and dJointSetFixed put it at a body's centre -- so the reference is given the joint as these calls
define it (ode_art) and its own conditioning and margin rules are asserted on that scene like on any other.  The ODE face has no
switch for the single-launch tick and no counters; which path ran is read from the batch's report in child processes, one that
leaves the choice to the batch and one with DMX_SMALL_TICK=0, which puts every world on the general path; the children make the
comparisons (run_named)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import joint_dense as jd
import lcp_dense as ld
import slider_dense as sd
import test_gpu_feedback as tf
import test_gpu_slider as sl
from __graft_entry__ import load_package, ROOT

pkg = load_package()
pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "rl-ode-physics_amd")
LIBS = [("libode_mi355.so", C.c_double), ("libode_mi355_single.so", C.c_float)]
H = 1.0 / 60.0
LO_STOP, HI_STOP, VEL, FMAX = 0, 1, 2, 5             # dParamLoStop, dParamHiStop, dParamVel, dParamFMax
MAXC = 8
SOFT_CFM = 0.0078125                   # (a float32 number)


def structs(real):
    V3 = real * 4

    class Surface(C.Structure):
        _fields_ = [("mode", C.c_int)] + [(n, real) for n in ("mu", "mu2", "rho", "rho2", "rhoN", "bounce", "bounce_vel", "soft_erp", "soft_cfm",
                                                              "motion1", "motion2", "motionN", "slip1", "slip2")]

    class Geom(C.Structure):
        _fields_ = [("pos", V3), ("normal", V3), ("depth", real), ("g1", C.c_void_p), ("g2", C.c_void_p), ("side1", C.c_int), ("side2", C.c_int)]

    class Contact(C.Structure):
        _fields_ = [("surface", Surface), ("geom", Geom), ("fdir1", V3)]

    class Feedback(C.Structure):
        _fields_ = [("f1", V3), ("t1", V3), ("f2", V3), ("t2", V3)]

    return Contact, Feedback


NEAR = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p)


def _bind(libname, real):
    pkg._lib.load()
    # (see tests/test_gpu_joints_ode.py: RTLD_DEEPBIND lets each of the two libraries call its own functions)
    lib = C.CDLL(os.path.join(PKG, libname), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    P, I = C.c_void_p, C.c_int
    R3 = C.POINTER(real)
    for name, res, args in (("dWorldCreate", P, []), ("dWorldDestroy", None, [P]), ("dWorldSetGravity", None, [P] + [real] * 3),
                            ("dWorldSetCFM", None, [P, real]), ("dWorldSetERP", None, [P, real]), ("dWorldStep", I, [P, real]),
                            ("dWorldQuickStep", I, [P, real]), ("dBodyCreate", P, [P]),
                            ("dWorldSetQuickStepNumIterations", None, [P, I]), ("dWorldSetQuickStepW", None, [P, real]),
                            ("dBodySetQuaternion", None, [P, R3]), ("dBodySetMass", None, [P, R3]), ("dBodySetKinematic", None, [P]),
                            ("dBodySetGyroscopicMode", None, [P, I]), ("dMassSetParameters", None, [R3] + [real] * 10),
                            ("dBodySetPosition", None, [P] + [real] * 3), ("dBodySetLinearVel", None, [P] + [real] * 3),
                            ("dBodySetAngularVel", None, [P] + [real] * 3), ("dBodyGetPosition", R3, [P]), ("dBodyGetQuaternion", R3, [P]),
                            ("dBodyGetLinearVel", R3, [P]), ("dBodyGetAngularVel", R3, [P]),
                            ("dJointCreateBall", P, [P, P]), ("dJointCreateHinge", P, [P, P]), ("dJointCreateSlider", P, [P, P]),
                            ("dJointCreateFixed", P, [P, P]), ("dJointCreateContact", P, [P, P, P]),
                            ("dJointAttach", None, [P, P, P]), ("dJointDestroy", None, [P]), ("dJointGetBody", P, [P, I]),
                            ("dJointSetBallAnchor", None, [P] + [real] * 3),
                            ("dJointSetHingeAnchor", None, [P] + [real] * 3), ("dJointSetHingeAxis", None, [P] + [real] * 3),
                            ("dJointSetHingeParam", None, [P, I, real]), ("dJointSetSliderAxis", None, [P] + [real] * 3),
                            ("dJointSetSliderParam", None, [P, I, real]), ("dJointSetFixed", None, [P]),
                            ("dJointSetFeedback", None, [P, P]), ("dJointGetFeedback", P, [P]),
                            ("dJointGroupCreate", P, [I]), ("dJointGroupEmpty", None, [P]),
                            ("dSimpleSpaceCreate", P, [P]), ("dCreatePlane", P, [P] + [real] * 4), ("dCreateBox", P, [P] + [real] * 3),
                            ("dGeomSetBody", None, [P, P]), ("dGeomGetBody", P, [P]), ("dSpaceCollide", None, [P, P, NEAR]),
                            ("dCollide", I, [P, P, I, P, I])):
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def body_state(lib, b):
    g = lambda f, n: np.array(getattr(lib, f)(b)[:n], np.float64)
    return g("dBodyGetPosition", 3), g("dBodyGetQuaternion", 4), g("dBodyGetLinearVel", 3), g("dBodyGetAngularVel", 3)


def bodies_of(lib, handles):
    st = [body_state(lib, b) for b in handles]
    n = len(handles)
    return ld.Bodies([s[0] for s in st], [s[1] for s in st], [s[2] for s in st], [s[3] for s in st], np.ones(n), np.ones((n, 3)))


class Scene:
    """unit bodies 0..5: 0 on a ball joint to the world, 1 on a motorised hinge to 0, 2 on a slider to the world attached as (0, body)
    and at its low stop, 3 welded to 2, 4 a box lying on the ground plane, 5 free.  feedback: which joints get a struct"""

    def __init__(self, lib, real, feedback=True, contacts_feedback=True):
        self.lib, self.real = lib, real
        self.Contact, self.Feedback = structs(real)
        w = self.w = lib.dWorldCreate()
        lib.dWorldSetGravity(w, 0.0, -9.8, 0.0)
        lib.dWorldSetCFM(w, 1e-5)
        lib.dWorldSetERP(w, 0.2)
        pos = [(0.0, 2.0, 0.0), (0.8, 2.0, 0.1), (-1.5, 1.5, 0.5), (-1.5, 2.3, 0.7), (3.0, 0.495, 0.0), (5.0, 3.0, 0.0)]
        self.b = [lib.dBodyCreate(w) for _ in pos]
        for b, p in zip(self.b, pos):
            lib.dBodySetPosition(b, *p)
        lib.dBodySetAngularVel(self.b[1], 0.2, -0.3, 0.4)
        lib.dBodySetLinearVel(self.b[2], 0.0, 0.3, 0.0)
        lib.dBodySetLinearVel(self.b[4], 0.1, -0.2, 0.0)
        ball = lib.dJointCreateBall(w, None)
        lib.dJointAttach(ball, self.b[0], None)
        lib.dJointSetBallAnchor(ball, 0.0, 2.5, 0.0)
        hinge = lib.dJointCreateHinge(w, None)
        lib.dJointAttach(hinge, self.b[1], self.b[0])
        lib.dJointSetHingeAnchor(hinge, 0.4, 2.0, 0.0)
        lib.dJointSetHingeAxis(hinge, 0.0, 0.0, 1.0)
        lib.dJointSetHingeParam(hinge, VEL, 1.0)
        lib.dJointSetHingeParam(hinge, FMAX, 2.0)
        slider = lib.dJointCreateSlider(w, None)
        lib.dJointAttach(slider, None, self.b[2])
        lib.dJointSetSliderAxis(slider, 0.0, 1.0, 0.0)
        lib.dJointSetSliderParam(slider, LO_STOP, 0.05)
        lib.dJointSetSliderParam(slider, HI_STOP, 1.0)
        weld = lib.dJointCreateFixed(w, None)
        lib.dJointAttach(weld, self.b[3], self.b[2])
        lib.dJointSetFixed(weld)
        self.joints = [ball, hinge, slider, weld]
        self.fb = [self.Feedback() for _ in self.joints]
        if feedback:
            for j, f in zip(self.joints, self.fb):
                assert lib.dJointGetFeedback(j) is None
                lib.dJointSetFeedback(j, C.addressof(f))
                assert lib.dJointGetFeedback(j) == C.addressof(f)
        self.space = lib.dSimpleSpaceCreate(None)
        self.plane = lib.dCreatePlane(self.space, 0.0, 1.0, 0.0, 0.0)
        box = lib.dCreateBox(self.space, 1.0, 1.0, 1.0)
        lib.dGeomSetBody(box, self.b[4])
        self.group = lib.dJointGroupCreate(0)
        self.contacts_feedback = contacts_feedback
        self.cfb, self.jts = [], []
        self.near = NEAR(self._near)
        # the same joints for the reference, in the sides as attached
        B = bodies_of(lib, self.b)
        self.art = np.array([jd.from_world(B, sd.BALL, 0, -1, (0.0, 2.5, 0.0)),
                             jd.from_world(B, sd.HINGE, 1, 0, (0.4, 2.0, 0.0), (0.0, 0.0, 1.0)),
                             jd.from_world(B, sd.SLIDER, -1, 2, B.pos[2], (0.0, 1.0, 0.0)),
                             jd.from_world(B, sd.FIXED, 3, 2, B.pos[2])], jd.ART_DTYPE)
        self.lim = sd.limots(B, self.art)
        sd.set_mode(self.lim[1], (-np.inf, np.inf, 1.0, 2.0))
        sd.set_mode(self.lim[2], (0.05, 1.0, 0.0, 0.0))

    def _near(self, data, o1, o2):
        lib = self.lib
        cs = (self.Contact * MAXC)()
        n = lib.dCollide(o1, o2, MAXC, C.addressof(cs) + self.Contact.geom.offset, C.sizeof(self.Contact))
        slot = {b: k for k, b in enumerate(self.b)}
        for k in range(n):
            # (frictionless, with a soft CFM: four normal rows on one body are one too many for its three degrees of freedom they
            #  act on, and kappa(A) ~ |A| h / cfm has to leave float32's 10 eps32 kappa under 1e-3)
            cs[k].surface.mode = 0x010                     # dContactSoftCFM
            cs[k].surface.mu = 0.0
            cs[k].surface.soft_cfm = SOFT_CFM
            c = lib.dJointCreateContact(self.w, self.group, C.addressof(cs) + k * C.sizeof(self.Contact))
            b1, b2 = lib.dGeomGetBody(o1), lib.dGeomGetBody(o2)
            lib.dJointAttach(c, b1, b2)
            f = self.Feedback()
            if self.contacts_feedback:
                lib.dJointSetFeedback(c, C.addressof(f))
            self.cfb.append(f)
            g = cs[k].geom
            self.jts.append((tuple(g.pos[:3]), tuple(g.normal[:3]), g.depth, slot.get(b1, -1), slot.get(b2, -1), 0x010, 0.0, 0, 0, 0, SOFT_CFM))

    def step(self, quick):
        """one tick -> (the bodies before it, the tick's contact joints, joint feedback [4, 4, 3] and contact feedback [n, 4, 3] in
        the sides as attached)"""
        lib = self.lib
        Bp = bodies_of(lib, self.b)
        self.cfb, self.jts = [], []
        lib.dSpaceCollide(self.space, None, self.near)
        assert (lib.dWorldQuickStep if quick else lib.dWorldStep)(self.w, H) == 1
        arr = lambda f: np.array([f.f1[:3], f.t1[:3], f.f2[:3], f.t2[:3]], np.float64)
        fj, fc = np.array([arr(f) for f in self.fb]), np.array([arr(f) for f in self.cfb]).reshape(-1, 4, 3)
        assert all(f.f1[3] == 0 and f.t1[3] == 0 and f.f2[3] == 0 and f.t2[3] == 0 for f in self.fb + self.cfb)
        jts = np.array(self.jts, ld.JOINT_DTYPE) if self.jts else np.zeros(0, ld.JOINT_DTYPE)
        lib.dJointGroupEmpty(self.group)
        return Bp, jts, fj, fc

    def close(self):
        self.lib.dWorldDestroy(self.w)


# ---------------------------------------------------------------------------------------------------------------------
# the scenes of test_gpu_feedback.py's cases 1 to 3, through the ODE calls
NOJ = np.zeros(0, ld.JOINT_DTYPE)
BOTH, EXACT_ONLY = (False, True), (False,)
ALL = tuple(n for n, _ in LIBS)


def named_scenes():
    """-> name: (B, art, lim, contact joints, ticks, quick-or-not of the steppers to run, small enough for the single-launch tick,
    the libraries to run it on).  The star on ground contacts runs on the double library only: with a slider's anchor where
    dJointSetSliderAxis puts it, at the spoke's centre and not half way to the hub, its island's 10 eps32 kappa(A) is 1.07e-3 to
    1.15e-3 for every seed from 0 to 11 -- above the 1e-3 up to which the float32 rule takes a scene for a test at all."""
    return {
        "one_body_per_mode": (*sd.one_body_per_mode(False, sl.MODE_SEED), NOJ, 1, BOTH, True, ALL),
        "one_body_per_mode_swapped": (*sd.one_body_per_mode(True, sl.MODE_SEED), NOJ, 1, BOTH, True, ALL),
        "one_body_fixed": (*sd.one_body(None, False, sl.MODE_SEED, kind=sd.FIXED), NOJ, 2, BOTH, True, ALL),
        "one_body_fixed_swapped": (*sd.one_body(None, True, sl.MODE_SEED, kind=sd.FIXED), NOJ, 2, BOTH, True, ALL),
        "all_kinds_chain": (*sd.all_kinds_chain(sl.CHAIN_SEED), NOJ, 1, BOTH, True, ALL),
        "small_world": (*sd.small_world(sl.WORLD_SEED), 3, BOTH, True, ALL),
        "star_8_on_the_ground": (*sd.star(8, seed=sl.STAR_GROUND_SEED, contacts=True), 1, BOTH, True, ALL[:1]),
        "star_40": (*sd.star(40, seed=sl.STAR_SEEDS[40]), 3, EXACT_ONLY, False, ALL),
        "star_100": (*sd.star(100, seed=sl.STAR_SEEDS[100]), 3, EXACT_ONLY, False, ALL),
    }


def ode_art(B, art):
    """the joints as the ODE calls define them at the poses B: a ball's and a hinge's anchor is the scene's, a slider's is the
    centre of dJointGetBody(j, 0) (dJointSetSliderAxis), a fixed joint's the centre of body 2, or of its one body (dJointSetFixed)"""
    out = []
    for a in art:
        b1, b2, kind = int(a["body1"]), int(a["body2"]), int(a["kind"])
        s, anchor, axis = (b1, a["anchor1"], a["axis1"]) if b1 >= 0 else (b2, a["anchor2"], a["axis2"])
        R = ld.quat_to_R(B.quat[s])
        at, ax = B.pos[s] + R @ anchor, R @ axis
        if kind == sd.SLIDER:
            at = B.pos[b1 if b1 >= 0 else b2]
        if kind == sd.FIXED:
            at = B.pos[b2 if b2 >= 0 else b1]
        out.append(jd.from_world(B, kind, b1, b2, at, ax))
    return np.array(out, jd.ART_DTYPE)


class Built:
    """an sd.* scene in an ODE world: .art / .lim are the joints and limots the calls made of it, for the reference"""

    def __init__(self, lib, real, B, art, lim, jts, W, feedback=True):
        self.lib, self.real, self.B0, self.jts, self.W = lib, real, B, jts, W
        self.Contact, self.Feedback = structs(real)
        rt = np.float32 if real is C.c_float else np.float64
        w = self.w = lib.dWorldCreate()
        lib.dWorldSetGravity(w, *[float(g) for g in W.gravity])
        lib.dWorldSetCFM(w, W.cfm)
        lib.dWorldSetERP(w, W.erp)
        lib.dWorldSetQuickStepNumIterations(w, W.iters)
        lib.dWorldSetQuickStepW(w, W.sor_w)
        self.mass, self.inertia = B.mass.astype(rt).astype(np.float64), B.inertia.astype(rt).astype(np.float64)
        self.b = []
        for s in range(B.n):
            b = lib.dBodyCreate(w)
            lib.dBodySetPosition(b, *B.pos[s])
            lib.dBodySetQuaternion(b, (real * 4)(*B.quat[s]))
            lib.dBodySetLinearVel(b, *B.lvel[s])
            lib.dBodySetAngularVel(b, *B.avel[s])
            m = (real * 17)()
            lib.dMassSetParameters(m, B.mass[s], 0.0, 0.0, 0.0, B.inertia[s][0], B.inertia[s][1], B.inertia[s][2], 0.0, 0.0, 0.0)
            lib.dBodySetMass(b, m)
            lib.dBodySetGyroscopicMode(b, 0)
            if B.flags[s] & ld.KINEMATIC:
                lib.dBodySetKinematic(b)
            self.b.append(b)
        Bq = self.bodies()
        self.art = ode_art(Bq, art)
        self.lim = sd.limots(Bq, self.art)
        h = lambda s: self.b[s] if s >= 0 else None
        self.joints = []
        for k, a in enumerate(art):
            b1, b2, kind = int(a["body1"]), int(a["body2"]), int(a["kind"])
            s = b1 if b1 >= 0 else b2
            R = ld.quat_to_R(Bq.quat[s])
            at = Bq.pos[s] + R @ (a["anchor1"] if b1 >= 0 else a["anchor2"])
            ax = R @ (a["axis1"] if b1 >= 0 else a["axis2"])
            create = {sd.BALL: lib.dJointCreateBall, sd.HINGE: lib.dJointCreateHinge, sd.SLIDER: lib.dJointCreateSlider, sd.FIXED: lib.dJointCreateFixed}[kind]
            j = create(w, None)
            lib.dJointAttach(j, h(b1), h(b2))
            if kind == sd.BALL:
                lib.dJointSetBallAnchor(j, *at)
            if kind == sd.HINGE:
                lib.dJointSetHingeAnchor(j, *at)
                lib.dJointSetHingeAxis(j, *ax)
            if kind == sd.SLIDER:
                lib.dJointSetSliderAxis(j, *ax)
            if kind == sd.FIXED:
                lib.dJointSetFixed(j)
            if kind in (sd.HINGE, sd.SLIDER):
                setp = lib.dJointSetHingeParam if kind == sd.HINGE else lib.dJointSetSliderParam
                for name, num in (("lo_stop", LO_STOP), ("hi_stop", HI_STOP), ("vel", VEL), ("fmax", FMAX)):
                    setp(j, num, float(lim[k][name]))
                    self.lim[k][name] = lim[k][name]
            self.joints.append(j)
        self.fb = [self.Feedback() for _ in self.joints]
        self.cfb = [self.Feedback() for _ in jts]
        self.feedback = feedback
        if feedback:
            for j, f in zip(self.joints, self.fb):
                lib.dJointSetFeedback(j, C.addressof(f))
        self.group = lib.dJointGroupCreate(0)

    def bodies(self):
        st = [body_state(self.lib, b) for b in self.b]
        return ld.Bodies([s[0] for s in st], [s[1] for s in st], [s[2] for s in st], [s[3] for s in st], self.mass, self.inertia, self.B0.flags)

    def step(self, quick):
        """one tick -> (the bodies before it, joint feedback [n, 4, 3] in the sides as given to the scene, contact feedback)"""
        lib = self.lib
        Bp = self.bodies()
        for k, j in enumerate(self.jts):
            ct = self.Contact()
            ct.surface.mode, ct.surface.mu = int(j["mode"]), float(j["mu"])
            ct.surface.bounce, ct.surface.bounce_vel = float(j["bounce"]), float(j["bounce_vel"])
            ct.surface.soft_erp, ct.surface.soft_cfm = float(j["soft_erp"]), float(j["soft_cfm"])
            for d in range(3):
                ct.geom.pos[d], ct.geom.normal[d] = float(j["pos"][d]), float(j["normal"][d])
            ct.geom.depth = float(j["depth"])
            c = lib.dJointCreateContact(self.w, self.group, C.addressof(ct))
            lib.dJointAttach(c, self.b[int(j["body1"])] if j["body1"] >= 0 else None, self.b[int(j["body2"])] if j["body2"] >= 0 else None)
            if self.feedback:
                lib.dJointSetFeedback(c, C.addressof(self.cfb[k]))
        assert (lib.dWorldQuickStep if quick else lib.dWorldStep)(self.w, self.W.h) == 1
        lib.dJointGroupEmpty(self.group)
        arr = lambda f: np.array([f.f1[:3], f.t1[:3], f.f2[:3], f.t2[:3]], np.float64)
        fj = np.array([arr(f) for f in self.fb]).reshape(-1, 4, 3)
        fc = np.array([arr(f) for f in self.cfb]).reshape(-1, 4, 3)
        # f1 / t1 belong to dJointGetBody(j, 0): a joint attached as (0, body) has the body there; the scene gave it second
        for k, a in enumerate(self.art):
            if a["body1"] < 0:
                assert lib.dJointGetBody(self.joints[k], 0) == self.b[int(a["body2"])] and np.all(fj[k][2:] == 0)
                fj[k] = fj[k][[2, 3, 0, 1]]
        for k, j in enumerate(self.jts):
            if j["body1"] < 0:
                fc[k] = fc[k][[2, 3, 0, 1]]
        return Bp, fj, fc

    def close(self):
        self.lib.dWorldDestroy(self.w)


def run_named(lib, real, name, quick):
    """the scene with a struct on every joint, and its twin with none: (a) and (b) by test_gpu_feedback.check_against_reference,
    (c) the twin's state is the same bit for bit"""
    B, art, lim, jts, ticks = named_scenes()[name][:5]
    prec = "float32" if real is C.c_float else "float64"
    W = tf.world()
    on, off = Built(lib, real, B, art, lim, jts, W), Built(lib, real, B, art, lim, jts, W, feedback=False)
    worst = [0.0]
    try:
        for _ in range(ticks):
            Bp, fj, fc = on.step(quick)
            off.step(quick)
            tf.check_against_reference(prec, "quick" if quick else "exact", W, Bp, jts, on.art, on.lim, fj, fc, worst)
            sa, sb = on.bodies(), off.bodies()
            for f in ("pos", "quat", "lvel", "avel"):
                assert np.array_equal(getattr(sa, f), getattr(sb, f)), f"(c) {f} differs with structs set"
            assert np.any(fj != 0) and all(np.all(np.array(f.f1[:3]) == 0) for f in off.fb)
    finally:
        on.close(); off.close()
    return worst[0]


@pytest.mark.parametrize("libname,real", LIBS)
@pytest.mark.parametrize("quick", [False, True])
def test_structs_are_filled_by_every_step(libname, real, quick):
    lib = _bind(libname, real)
    sc = Scene(lib, real)
    prec = "float32" if real is C.c_float else "float64"
    W = ld.World(h=H, gravity=(0.0, -9.8, 0.0), erp=0.2, cfm=1e-5)
    worst = [0.0]
    try:
        for _ in range(3):
            Bp, jts, fj, fc = sc.step(quick)
            assert len(jts) >= 3, "the box should lie on the plane"
            # f1 / t1 belong to dJointGetBody(j, 0): the slider attached as (0, body) has the body there, the world's zeros second
            assert lib.dJointGetBody(sc.joints[2], 0) == sc.b[2] and np.any(fj[2][0] != 0) and np.all(fj[2][2:] == 0)
            given = fj.copy()
            given[2] = fj[2][[2, 3, 0, 1]]                 # (the reference's joint is (world, body): the sides as attached)
            tf.check_against_reference(prec, "quick" if quick else "exact", W, Bp, jts, sc.art, sc.lim, given, fc, worst)
            assert np.all(fj[0][2:] == 0) and fj[0][0][1] > 0          # the ball joint carries bodies 0 and 1; the world side: zeros
            box_first = jts["body1"] == 4
            assert np.all(fc[box_first, 2:] == 0) and np.all(fc[~box_first, :2] == 0) and np.sum(fc[:, 0::2, 1]) > 0
    finally:
        sc.close()


@pytest.mark.parametrize("libname,real", LIBS)
def test_forgetting_a_struct_and_destroying_a_joint(libname, real):
    """dJointSetFeedback(j, 0) stops the filling; a joint destroyed with a struct set takes it off the world's count, and when the
    last struct is gone the state goes on bit for bit as in a world that never had one"""
    lib = _bind(libname, real)
    a, b = Scene(lib, real), Scene(lib, real, feedback=False, contacts_feedback=False)
    try:
        a.step(False); b.step(False)
        assert np.any(np.array(a.fb[1].f1[:3]) != 0) and all(f.f1[1] == 0 for f in b.fb)
        lib.dJointSetFeedback(a.joints[1], None)
        before = list(a.fb[1].f1[:3])
        a.step(False); b.step(False)
        assert list(a.fb[1].f1[:3]) == before and lib.dJointGetFeedback(a.joints[1]) is None
        for j in (a.joints[0], a.joints[2], a.joints[3]):
            lib.dJointSetFeedback(j, None)
        a.contacts_feedback = False
        for _ in range(2):
            a.step(False); b.step(False)
        sa, sb = bodies_of(lib, a.b), bodies_of(lib, b.b)
        for f in ("pos", "quat", "lvel", "avel"):
            assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
    finally:
        a.close(); b.close()


def _grown(lib, real):
    """a world that outgrows its batch (the 513th body) with structs set: the new batch is told to report feedback again"""
    sc = Scene(lib, real)
    prec = "float32" if real is C.c_float else "float64"
    W = ld.World(h=H, gravity=(0.0, -9.8, 0.0), erp=0.2, cfm=1e-5)
    try:
        sc.step(False)
        for k in range(513 - len(sc.b)):
            lib.dBodySetPosition(lib.dBodyCreate(sc.w), 10.0 + 2.0 * (k % 32), 50.0, 2.0 * (k // 32))
        for quick in (False, True):
            Bp, jts, fj, fc = sc.step(quick)
            given = fj.copy()
            given[2] = fj[2][[2, 3, 0, 1]]
            tf.check_against_reference(prec, "quick" if quick else "exact", W, Bp, jts, sc.art, sc.lim, given, fc, [0.0])
            assert len(fc) >= 3 and np.any(fc != 0)
    finally:
        sc.close()


def _child(libname, what):
    real = dict(LIBS)[libname]
    lib = _bind(libname, real)
    if what == "grow":
        return _grown(lib, real)
    if what in ("named", "named_small"):
        for name, v in named_scenes().items():
            if (what == "named_small" and not v[6]) or libname not in v[7]:
                continue
            for quick in v[5]:
                print(f"scene {name} quick={int(quick)} ticks={v[4]}", file=sys.stderr, flush=True)
                run_named(lib, real, name, quick)
        return
    for with_structs in (False, True):
        sc = Scene(lib, real, feedback=with_structs, contacts_feedback=with_structs)
        for _ in range(3):
            sc.step(False)
        sc.step(True)
        sc.close()


def _run_child(libname, what, **env):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), libname, what], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DMX_SMALL_TICK_REPORT": "1", "PYTHONPATH": os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **env})
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-2500:]
    return p.stderr


@pytest.mark.parametrize("libname,real", LIBS)
def test_the_path_is_the_one_it_was(libname, real):
    """a process of its own (the batch reports its counters on stderr when it is destroyed, DMX_SMALL_TICK_REPORT, a switch read once
    per process): four ticks of the scene are four single-launch ticks in a world with no struct set, as they always were, and in
    the next world, with structs set, as well"""
    err = _run_child(libname, "paths")
    lines = re.findall(r"small tick: small=(\d+) general=(\d+)", err)
    assert lines == [("4", "0"), ("4", "0")], err[-1000:]


def _paths(err):
    """-> [(scene line, [(small, general) of the world with structs, of its twin])]"""
    out = []
    for line in err.splitlines():
        m = re.match(r"scene (\S+) quick=(\d) ticks=(\d+)", line)
        if m:
            out.append(((m.group(1), int(m.group(2)), int(m.group(3))), []))
        m = re.search(r"small tick: small=(\d+) general=(\d+)", line)
        if m and out:
            out[-1][1].append((int(m.group(1)), int(m.group(2))))
    return out


@pytest.mark.parametrize("libname,real", LIBS)
def test_the_named_scenes_on_the_path_the_batch_chooses(libname, real):
    """the named scenes through the ODE calls (run_named), and which path they take when the choice is the batch's: the small worlds
    the single-launch tick, every tick of them; a world with structs set the same path as its twin without"""
    got = _paths(_run_child(libname, "named"))
    scenes = named_scenes()
    assert [g[0][0] for g in got] == [n for n, v in scenes.items() if libname in v[7] for _ in v[5]]
    for (name, quick, ticks), worlds in got:
        assert len(worlds) == 2 and worlds[0] == worlds[1] and sum(worlds[0]) == ticks, (name, quick, worlds)
        if scenes[name][6]:
            assert worlds[0] == (ticks, 0), (name, quick, worlds)


@pytest.mark.parametrize("libname,real", LIBS)
def test_the_small_scenes_on_the_general_path(libname, real):
    """DMX_SMALL_TICK=0: the same worlds, the same comparisons, every tick on the general path -- its kernel and the copy back
    behind dJointSetFeedback"""
    got = _paths(_run_child(libname, "named_small", DMX_SMALL_TICK="0"))
    assert len(got) == sum(len(v[5]) for v in named_scenes().values() if v[6] and libname in v[7])
    for (name, quick, ticks), worlds in got:
        assert worlds == [(0, ticks), (0, ticks)], (name, quick, worlds)


@pytest.mark.parametrize("libname,real", LIBS)
def test_a_world_that_grows_keeps_filling_the_structs(libname, real):
    """in a process of its own: an error of the batch ends the process behind the ODE calls"""
    _run_child(libname, "grow")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
