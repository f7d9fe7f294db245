"""BatchWorld: Python view of one dmxBatch (include/dmx_batch.h).

Mirrors the reference's physics-facing calls in batch form: world setup
(main.c:94-98), AddBody (main.c:695-733), the tick loop (main.c:211-215) and
the pose read-back (main.c:221-237), all through the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib

DMX_F32, DMX_F64 = 0, 1
POS, QUAT, LVEL, AVEL, MASS, INERTIA, SIDES, FORCE, TORQUE = range(9)
QUAT_RAW, STATE = 9, 10      # quaternion stored as given; pos3 quat4 lvel3 avel3 in one piece
_K = {POS: 3, QUAT: 4, LVEL: 3, AVEL: 3, MASS: 1, INERTIA: 3, SIDES: 3, FORCE: 3, TORQUE: 3, QUAT_RAW: 4, STATE: 13}
GEOM_NONE, GEOM_SPHERE, GEOM_BOX = 0, 1, 2
GYRO_OFF, GYRO_EXPLICIT, GYRO_IMPLICIT = 0, 1, 2
CONTACT_BOUNCE = 0x004
SNAPSHOT_PINGPONG, SNAPSHOT_COPY = 0, 1
EXACT_AUTO, EXACT_STAGED, EXACT_ONE_WORKGROUP = 0, 1, 2
STEPPER_QUICK, STEPPER_EXACT = 0, 1
ORDER_CREATION, ORDER_ODE = 0, 1
BODY_ALIVE, BODY_KINEMATIC, BODY_NOGRAVITY, BODY_NOGYRO = 1, 2, 4, 8
BODY_AUTODISABLE, BODY_DISABLED = 16, 32      # auto-disable: may fall asleep by itself / is asleep
AUTO_DISABLE_STATS = ("asleep", "islands_skipped", "slept", "woken")
# dmxBodyDamping (include/dmx_batch.h): five doubles per slot; the defaults are 0, 0, 0.01, 0.01, inf
BODY_DAMPING_DTYPE = np.dtype([("lin_scale", "<f8"), ("ang_scale", "<f8"), ("lin_threshold", "<f8"), ("ang_threshold", "<f8"),
                               ("max_angular_speed", "<f8")])
CONTACT_SOFT_ERP, CONTACT_SOFT_CFM = 0x008, 0x010
CONTACT_APPROX1_1, CONTACT_APPROX1_2, CONTACT_APPROX1 = 0x1000, 0x2000, 0x3000      # friction bounded by mu times the normal force
# dmxContactJoint (include/dmx_batch.h): the C layout, padding included (tests/test_solver_dense.py checks it with offsetof)
CONTACT_JOINT_DTYPE = np.dtype({
    "names": ["pos", "normal", "depth", "body1", "body2", "mode", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"],
    "formats": [(np.float64, 3), (np.float64, 3), np.float64, np.int32, np.int32, np.int32, np.float64, np.float64,
                np.float64, np.float64, np.float64],
    "offsets": [0, 24, 48, 56, 60, 64, 72, 80, 88, 96, 104],
    "itemsize": 112})
# dmxContactSurface (include/dmx_batch.h): the rest of ODE's contact surface, one per contact joint (step_joints' `surfaces`); bit X
# of a joint's mode says that field X of its surface is read.  The bits' values are ODE's.
CONTACT_MU2, CONTACT_FDIR1, CONTACT_MOTION1, CONTACT_MOTION2, CONTACT_MOTIONN = 0x001, 0x002, 0x020, 0x040, 0x080
CONTACT_SLIP1, CONTACT_SLIP2 = 0x100, 0x200
CONTACT_SURFACE_EXT = 0x3e3
CONTACT_SURFACE_DTYPE = np.dtype({
    "names": ["mu2", "fdir1", "motion1", "motion2", "motionN", "slip1", "slip2"],
    "formats": [np.float64, (np.float64, 3), np.float64, np.float64, np.float64, np.float64, np.float64],
    "offsets": [0, 8, 32, 40, 48, 56, 64],
    "itemsize": 72})
# dmxJoint (include/dmx_batch.h): an articulation joint -- a ball, a hinge, a slider or a fixed joint -- of the persistent set
# (set_joints)
JOINT_BALL, JOINT_HINGE, JOINT_SLIDER, JOINT_FIXED = 1, 2, 3, 4
JOINT_DTYPE = np.dtype({
    "names": ["kind", "body1", "body2", "reserved", "anchor1", "anchor2", "axis1", "axis2"],
    "formats": [np.int32, np.int32, np.int32, np.int32, (np.float64, 3), (np.float64, 3), (np.float64, 3), (np.float64, 3)],
    "offsets": [0, 4, 8, 12, 16, 40, 64, 88],
    "itemsize": 112})
# dmxHingeLimot (include/dmx_batch.h): a hinge's or a slider's stops, motor and zero pose (a fixed joint's zero pose) -- one entry per
# joint of the set (set_hinge_limots)
HINGE_LIMOT_DTYPE = np.dtype({
    "names": ["lo_stop", "hi_stop", "vel", "fmax", "qrel0"],
    "formats": [np.float64, np.float64, np.float64, np.float64, (np.float64, 4)],
    "offsets": [0, 8, 16, 24, 32],
    "itemsize": 64})
# dmxAMotor (include/dmx_batch.h; _lib.dmxAMotor is the same layout): an angular motor -- a joint of kind JOINT_AMOTOR -- one entry
# per joint of the set (set_amotors)
JOINT_AMOTOR = 5
AMOTOR_USER, AMOTOR_EULER = 0, 1
AMOTOR_DTYPE = np.dtype({
    "names": ["mode", "num_axes", "rel", "pad", "axis", "ref1", "ref2", "angle", "lo_stop", "hi_stop", "vel", "fmax"],
    "formats": [np.int32, np.int32, (np.int32, 3), np.int32, (np.float64, (3, 3)), (np.float64, 3), (np.float64, 3), (np.float64, 3),
                (np.float64, 3), (np.float64, 3), (np.float64, 3), (np.float64, 3)],
    "offsets": [0, 4, 8, 20, 24, 96, 120, 144, 168, 192, 216, 240],
    "itemsize": 264})
LCP_STATS = ("solves", "rounds", "max_rounds", "last_m", "last_nu", "last_nbd", "single", "fallback")
# the single-launch tick of small worlds (dmxBatchSetSmallTick); the counters of dmxBatchSmallTickStats, in its order: ticks on
# that path, step_joints ticks on the general path, then one count per reason a tick was not eligible
SMALL_TICK_OFF, SMALL_TICK_AUTO = 0, 1
SMALL_TICK_STATS = ("small", "general", "mode", "row_order", "subset", "bodies", "islands", "sor_rows", "lds_fit")
# ray casts (dmxBatchRayCast): result ids below zero, the visibility mask's bits, the forms
RAY_MISS, RAY_PLANE = -1, -2           # static box k: -3 - k
RAY_SPHERES, RAY_BOXES, RAY_CONVEX, RAY_STATIC, RAY_PLANE_BIT, RAY_ALL = 1, 2, 4, 8, 16, 31
RAY_FORM_AUTO, RAY_FORM_LANE, RAY_FORM_WAVE, RAY_FORM_BRUTE = 0, 1, 2, 3


class DmxError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def _check(rc, what):
    if rc != 0:
        raise DmxError(f"{what} failed with code {rc}", rc)


class BatchWorld:
    def __init__(self, n_bodies, dtype="float32", device=0, gravity=(0.0, -9.8, 0.0)):
        self.lib = _lib.load()
        self.dtype = np.dtype(dtype)
        prec = {4: DMX_F32, 8: DMX_F64}[self.dtype.itemsize]
        self.n = int(n_bodies)
        h = C.c_void_p()
        _check(self.lib.dmxBatchCreate(C.byref(h), self.n, prec, device), "dmxBatchCreate")
        self.h = h
        self.set_gravity(*gravity)       # dWorldSetGravity(world, 0, -9.8, 0)  main.c:96

    # -- lifecycle -----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.dmxBatchDestroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- parameters ------------------------------------------------------------
    def set_gravity(self, x, y, z):
        _check(self.lib.dmxBatchSetGravity(self.h, x, y, z), "dmxBatchSetGravity")

    def set_erp(self, erp):
        _check(self.lib.dmxBatchSetERP(self.h, erp), "dmxBatchSetERP")

    def set_cfm(self, cfm):
        _check(self.lib.dmxBatchSetCFM(self.h, cfm), "dmxBatchSetCFM")

    def set_quickstep(self, iters, sor_w=1.3):
        _check(self.lib.dmxBatchSetQuickStep(self.h, iters, sor_w), "dmxBatchSetQuickStep")

    def set_gyro_mode(self, mode):
        _check(self.lib.dmxBatchSetGyroMode(self.h, mode), "dmxBatchSetGyroMode")

    def set_surface(self, mode=CONTACT_BOUNCE, mu=float("inf"), bounce=0.2, bounce_vel=0.1):
        _check(self.lib.dmxBatchSetSurface(self.h, mode, mu, bounce, bounce_vel), "dmxBatchSetSurface")

    def set_max_contacts(self, n):
        _check(self.lib.dmxBatchSetMaxContacts(self.h, n), "dmxBatchSetMaxContacts")

    def set_plane(self, a, b, c, d, enable=True):
        _check(self.lib.dmxBatchSetPlane(self.h, a, b, c, d, int(enable)), "dmxBatchSetPlane")

    # -- data ----------------------------------------------------------------------
    def upload(self, field, arr, first=0):
        a = np.ascontiguousarray(arr, dtype=self.dtype).reshape(-1, _K[field])
        _check(self.lib.dmxBatchUpload(self.h, field, a.ctypes.data, first, a.shape[0]), "dmxBatchUpload")

    def download(self, field, first=0, count=None):
        count = self.n - first if count is None else count
        out = np.empty((count, _K[field]), self.dtype)
        _check(self.lib.dmxBatchDownload(self.h, field, out.ctypes.data, first, count), "dmxBatchDownload")
        return out

    def upload_geom_type(self, types, first=0):
        t = np.ascontiguousarray(types, dtype=np.uint8)
        _check(self.lib.dmxBatchUploadGeomType(self.h, t.ctypes.data, first, t.shape[0]), "dmxBatchUploadGeomType")

    def set_static_boxes(self, boxes):
        """AddBodyMap (main.c:735-761): `boxes` = [(sides3, pos3, R12)], the static floor / walls, e.g. scenes.reference_map()"""
        n = len(boxes)
        sides = np.ascontiguousarray([b[0] for b in boxes], dtype=np.float64).reshape(n, 3)
        pos = np.ascontiguousarray([b[1] for b in boxes], dtype=np.float64).reshape(n, 3)
        rot = np.ascontiguousarray([b[2] for b in boxes], dtype=np.float64).reshape(n, 12)
        _check(self.lib.dmxBatchSetStaticBoxes(self.h, n, sides.ctypes.data, pos.ctypes.data, rot.ctypes.data),
               "dmxBatchSetStaticBoxes")

    def set_convex_hull(self, points):
        """Body-frame points of the hull every GEOM_CONVEX body uses; returns the hull's bounding radius (upload it as
        sides[:, 0] of the convex bodies)."""
        p = np.ascontiguousarray(points, dtype=np.float64)
        r = C.c_double()
        _check(self.lib.dmxBatchSetConvexHull(self.h, p.shape[0], p.ctypes.data, C.byref(r)), "dmxBatchSetConvexHull")
        return r.value

    def set_convex_hull_faces(self, planes):
        """the hull's faces (nf x 4: unit outward normal, offset; body frame), e.g. hull.planes(points)"""
        pl = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        _check(self.lib.dmxBatchSetConvexHullFaces(self.h, pl.shape[0], pl.ctypes.data), "dmxBatchSetConvexHullFaces")

    def load_scene(self, scene):
        """Upload a scenes.Scene (the batch form of the AddBody loop, main.c:695-733)."""
        self.upload(POS, scene.pos)
        self.upload(QUAT, scene.quat)
        self.upload(LVEL, scene.lvel)
        self.upload(AVEL, scene.avel)
        self.upload(MASS, scene.mass)
        self.upload(INERTIA, scene.inertia)
        if getattr(scene, "hull_points", None) is not None:
            self.set_convex_hull(scene.hull_points)
            if getattr(scene, "hull_planes", None) is not None:
                self.set_convex_hull_faces(scene.hull_planes)
        self.upload(SIDES, scene.sides)
        self.upload_geom_type(scene.gtype)
        if scene.plane is not None:
            self.set_plane(*scene.plane, enable=True)
        if getattr(scene, "static_boxes", None):
            self.set_static_boxes(scene.static_boxes)

    # -- checkpoint / resume ---------------------------------------------------------------------------------
    def checkpoint(self):
        """The per-body data a later `restore` needs to continue bit for bit: the 13-real state, the force / torque
        accumulators and the per-body constants (mass, inertia, extents).  NOT in it: geometry classes, the hull, static
        boxes, plane, gravity, solver and surface parameters, active count -- a fresh batch is set up from the scene first,
        then restored.  (The reference keeps no resumable state -- its 60 Hz snapshot holds poses only, SURVEY section 5 --
        so this is new surface, built on Download.)"""
        self.synchronize()
        return {"state": self.download(STATE), "force": self.download(FORCE), "torque": self.download(TORQUE),
                "mass": self.download(MASS), "inertia": self.download(INERTIA), "sides": self.download(SIDES)}

    def restore(self, ckpt):
        self.upload(MASS, ckpt["mass"]); self.upload(INERTIA, ckpt["inertia"]); self.upload(SIDES, ckpt["sides"])
        self.upload(STATE, ckpt["state"])                    # stored as given: no renormalisation of the quaternions
        # always, zeros included: accumulators added to the live batch since the checkpoint must not act after the restore
        self.upload(FORCE, ckpt["force"]); self.upload(TORQUE, ckpt["torque"])

    def state(self):
        return (self.download(POS), self.download(QUAT), self.download(LVEL), self.download(AVEL))

    def device_ptr(self, field, comp):
        return self.lib.dmxBatchDevicePtr(self.h, field, comp)

    @property
    def stride(self):
        return self.lib.dmxBatchStride(self.h)

    # -- stepping ----------------------------------------------------------------------
    def step(self, h, nsteps=1):
        _check(self.lib.dmxBatchStep(self.h, h, nsteps), "dmxBatchStep")

    # -- explicit contact joints: the callback form of the tick (dJointCreateContact + dWorldStep, include/dmx_batch.h) --
    def step_joints(self, h, joints, surfaces=None):
        """one tick driven by `joints`, an array of CONTACT_JOINT_DTYPE (or anything with its fields); `surfaces`: one
        CONTACT_SURFACE_DTYPE per joint, whose fields are read where the joint's mode has their bit (dmxBatchStepJointsSurface)"""
        j = np.ascontiguousarray(np.asarray(joints).astype(CONTACT_JOINT_DTYPE, copy=False))
        if surfaces is None:
            _check(self.lib.dmxBatchStepJoints(self.h, h, j.shape[0], j.ctypes.data if j.shape[0] else None),
                   "dmxBatchStepJoints")
        else:
            s = np.ascontiguousarray(np.asarray(surfaces).astype(CONTACT_SURFACE_DTYPE, copy=False))
            if s.shape[0] != j.shape[0]:
                raise ValueError("step_joints: %d surfaces for %d joints" % (s.shape[0], j.shape[0]))
            # (an empty array has no address worth passing; one spare entry keeps `surfaces` non-NULL, which is what selects the call)
            if s.shape[0] == 0:
                s = np.zeros(1, CONTACT_SURFACE_DTYPE)
            _check(self.lib.dmxBatchStepJointsSurface(self.h, h, j.shape[0], j.ctypes.data if j.shape[0] else None, s.ctypes.data),
                   "dmxBatchStepJointsSurface")
        self._last_n_joints = int(j.shape[0])

    # -- articulation joints: ball, hinge, slider and fixed (dJointCreateBall / Hinge / Slider / Fixed), a set that persists
    #    between ticks --
    def set_joints(self, arr):
        """replace the set of articulation joints (an array of JOINT_DTYPE; empty or None removes it); every later
        step_joints tick honours them, ahead of the tick's contact joints"""
        j = np.zeros(0, JOINT_DTYPE) if arr is None else np.ascontiguousarray(np.asarray(arr).astype(JOINT_DTYPE, copy=False)).reshape(-1)
        _check(self.lib.dmxBatchSetJoints(self.h, j.shape[0], j.ctypes.data if j.shape[0] else None), "dmxBatchSetJoints")

    def joint_count(self):
        return int(self.lib.dmxBatchJointCount(self.h))

    def joint_from_world(self, kind, body1, body2, anchor, axis=None):
        """a JOINT_DTYPE record from a world-frame anchor (and axis, for a hinge or a slider: a slider's anchor is any point of
        its line) at the bodies' current poses; -1 = the world"""
        out = np.zeros(1, JOINT_DTYPE)
        a = np.ascontiguousarray(anchor, np.float64).reshape(3)
        x = None if axis is None else np.ascontiguousarray(axis, np.float64).reshape(3)
        _check(self.lib.dmxBatchJointFromWorld(self.h, int(kind), int(body1), int(body2), a.ctypes.data,
                                               None if x is None else x.ctypes.data, out.ctypes.data), "dmxBatchJointFromWorld")
        return out[0]

    def joint_errors(self):
        """-> (pos_err [n], axis_err [n], (max pos_err, max axis_err)) of the set at the current state: the anchors' separation
        and, for hinges, |u x w|, computed on the device.  A slider: the separation across its axis and |2 e_v|, the rotation
        away from its zero pose; a fixed joint: the separation and |2 e_v|"""
        n = self.joint_count()
        pe, ae, mx = np.zeros(n), np.zeros(n), np.zeros(2)
        _check(self.lib.dmxBatchJointErrors(self.h, pe.ctypes.data if n else None, ae.ctypes.data if n else None, mx.ctypes.data),
               "dmxBatchJointErrors")
        return pe, ae, (float(mx[0]), float(mx[1]))

    # -- the hinges' limits, motors and angles (dJointSetHingeParam, dJointGetHingeAngle / Rate) --
    def set_hinge_limots(self, arr):
        """the hinges' and sliders' stops and motors (a slider's in metres, m/s and N) and the zero poses of hinges, sliders and
        fixed joints: an array of HINGE_LIMOT_DTYPE, one entry per joint of the set (a ball's is ignored); empty or None removes
        them.  May be replaced every tick; set_joints drops them"""
        l = np.zeros(0, HINGE_LIMOT_DTYPE) if arr is None else np.ascontiguousarray(np.asarray(arr).astype(HINGE_LIMOT_DTYPE, copy=False)).reshape(-1)
        _check(self.lib.dmxBatchSetHingeLimots(self.h, l.shape[0], l.ctypes.data if l.shape[0] else None), "dmxBatchSetHingeLimots")

    def hinge_limot_init(self, joint):
        """a HINGE_LIMOT_DTYPE record without stops or motor whose zero pose is the bodies' current one"""
        j = np.ascontiguousarray(np.asarray(joint).astype(JOINT_DTYPE, copy=False)).reshape(1)
        out = np.zeros(1, HINGE_LIMOT_DTYPE)
        _check(self.lib.dmxBatchHingeLimotInit(self.h, j.ctypes.data, out.ctypes.data), "dmxBatchHingeLimotInit")
        return out[0]

    def hinge_angles(self):
        """-> (theta [n], theta_dot [n]) of the set's joints at the current state, computed on the device (balls and inactive
        joints: 0); without limots the angle is relative to the two frames coinciding"""
        n = self.joint_count()
        th, rate = np.zeros(n), np.zeros(n)
        _check(self.lib.dmxBatchHingeAngles(self.h, th.ctypes.data if n else None, rate.ctypes.data if n else None), "dmxBatchHingeAngles")
        return th, rate

    def slider_positions(self):
        """-> (s [n], s_dot [n]) of the set's joints at the current state, computed on the device (other kinds and inactive
        joints: 0): the position of side 1 against side 2 along the axis, zero where the two anchors meet"""
        n = self.joint_count()
        s, rate = np.zeros(n), np.zeros(n)
        _check(self.lib.dmxBatchSliderPositions(self.h, s.ctypes.data if n else None, rate.ctypes.data if n else None), "dmxBatchSliderPositions")
        return s, rate

    # -- angular motors (dJointCreateAMotor): joints of kind JOINT_AMOTOR, their data in a table beside the set --
    def set_amotors(self, arr):
        """the angular motors' modes, axes, angles, stops and motors: an array of AMOTOR_DTYPE, one entry per joint of the set
        (only an AMotor's is read); empty or None removes them.  May be replaced every tick; set_joints drops them"""
        m = np.zeros(0, AMOTOR_DTYPE) if arr is None else np.ascontiguousarray(np.asarray(arr).astype(AMOTOR_DTYPE, copy=False)).reshape(-1)
        _check(self.lib.dmxBatchSetAMotors(self.h, m.shape[0], m.ctypes.data if m.shape[0] else None), "dmxBatchSetAMotors")

    def amotor_from_world(self, body1, body2, mode, axes, rel=(0, 0, 0), num_axes=None):
        """an AMOTOR_DTYPE record from world-frame axes (up to three rows) at the bodies' current poses; -1 = the world.  Euler
        mode takes axes 0 and 2 (perpendicular) and makes the current pose angles zero; stops -+inf, no motor"""
        ax = np.zeros((3, 3))
        a = np.atleast_2d(np.asarray(axes, np.float64))
        ax[:a.shape[0]] = a
        n = int(a.shape[0] if num_axes is None else num_axes)
        r = np.ascontiguousarray(rel, np.int32).reshape(3)
        out = np.zeros(1, AMOTOR_DTYPE)
        _check(self.lib.dmxBatchAMotorFromWorld(self.h, int(body1), int(body2), int(mode), n, r.ctypes.data, ax.ctypes.data, out.ctypes.data),
               "dmxBatchAMotorFromWorld")
        return out[0]

    def amotor_angles(self):
        """-> (theta [n, 3], rate [n, 3]) of the set's joints at the current state, computed on the device by the kernel that
        prepares a tick's AMotor rows (other kinds, unused axes and inactive joints: 0).  The rate is a_i . (omega_1 - omega_2),
        the velocity the axis's row acts on; user mode echoes the supplied angles"""
        n = self.joint_count()
        th, rate = np.zeros((n, 3)), np.zeros((n, 3))
        _check(self.lib.dmxBatchAMotorAngles(self.h, th.ctypes.data if n else None, rate.ctypes.data if n else None), "dmxBatchAMotorAngles")
        return th, rate

    # -- feedback: what every joint and contact joint applied in the last tick (dJointSetFeedback) --
    def set_feedback(self, on):
        """on: every later step_joints tick leaves the force and torque each joint and contact joint applied (default off)"""
        _check(self.lib.dmxBatchSetFeedback(self.h, int(bool(on))), "dmxBatchSetFeedback")

    def joint_feedback(self):
        """-> [n, 4, 3] float64: f1, t1, f2, t2 per joint of the set, in the sides as given (include/dmx_batch.h)"""
        n = self.joint_count()
        out = np.zeros((n, 4, 3))
        _check(self.lib.dmxBatchJointFeedback(self.h, out.ctypes.data if n else None), "dmxBatchJointFeedback")
        return out

    def contact_feedback(self, n=None):
        """-> [n, 4, 3] float64: f1, t1, f2, t2 per contact joint of the last step_joints tick, in the order given; n = how
        many that tick was given (default: what this object's last step_joints call was given)"""
        n = int(getattr(self, "_last_n_joints", 0) if n is None else n)
        out = np.zeros((n, 4, 3))
        _check(self.lib.dmxBatchContactFeedback(self.h, n, out.ctypes.data if n else None), "dmxBatchContactFeedback")
        return out

    def feedback_device(self):
        """-> (joints, contacts): device addresses of the last tick's feedback, 12 reals per entry in the batch's precision,
        valid until the next tick"""
        a, c = C.c_void_p(), C.c_void_p()
        _check(self.lib.dmxBatchFeedbackDevice(self.h, C.byref(a), C.byref(c)), "dmxBatchFeedbackDevice")
        return a.value, c.value

    def set_stepper(self, stepper):
        """STEPPER_QUICK (dWorldQuickStep, default) / STEPPER_EXACT (dWorldStep) for step_joints"""
        _check(self.lib.dmxBatchSetStepper(self.h, int(stepper)), "dmxBatchSetStepper")

    def lcp_stats(self):
        """the eight counters of the grid-wide exact solve (LCP_STATS names them)"""
        out = (C.c_int64 * 8)()
        _check(self.lib.dmxBatchLcpStats(self.h, out), "dmxBatchLcpStats")
        return dict(zip(LCP_STATS, out))

    def set_small_tick(self, mode):
        """SMALL_TICK_AUTO (default): an eligible step_joints tick runs as one kernel launch; SMALL_TICK_OFF: never"""
        _check(self.lib.dmxBatchSetSmallTick(self.h, int(mode)), "dmxBatchSetSmallTick")

    def small_tick_stats(self):
        """ticks per path and per reason a tick was not eligible (SMALL_TICK_STATS names them)"""
        out = (C.c_int64 * len(SMALL_TICK_STATS))()
        _check(self.lib.dmxBatchSmallTickStats(self.h, out), "dmxBatchSmallTickStats")
        return dict(zip(SMALL_TICK_STATS, out))

    def upload_body_flags(self, flags, first=0):
        """BODY_ALIVE / BODY_KINEMATIC / BODY_NOGRAVITY / BODY_NOGYRO per slot (uint8).  step_joints honours them; step,
        step_timed, step_range, chunk_tick(s) and exact_tick refuse (DmxError, DMX_EINVAL) while an active slot is not plain
        BODY_ALIVE (include/dmx_batch.h)"""
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        _check(self.lib.dmxBatchUploadBodyFlags(self.h, f.ctypes.data, first, f.shape[0]), "dmxBatchUploadBodyFlags")

    # -- auto-disable: resting bodies sleep, islands wake on contact (include/dmx_batch.h, "auto-disable") --
    def set_auto_disable(self, lin_threshold=0.01, ang_threshold=0.01, idle_steps=10, idle_time=0.0):
        """the batch's thresholds (m/s, rad/s) and idle counters for bodies that carry BODY_AUTODISABLE; resets every slot's
        counters.  step_joints only"""
        _check(self.lib.dmxBatchSetAutoDisable(self.h, float(lin_threshold), float(ang_threshold), int(idle_steps), float(idle_time)),
               "dmxBatchSetAutoDisable")

    def auto_disable(self):
        """-> (lin_threshold, ang_threshold, idle_steps, idle_time)"""
        a, b, t, s = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        _check(self.lib.dmxBatchGetAutoDisable(self.h, C.byref(a), C.byref(b), C.byref(s), C.byref(t)), "dmxBatchGetAutoDisable")
        return a.value, b.value, s.value, t.value

    def body_flags(self):
        """-> [n] uint8: the flag bytes as they stand after every tick enqueued so far (BODY_DISABLED: asleep)"""
        out = np.zeros(self.n, np.uint8)
        _check(self.lib.dmxBatchDownloadBodyFlags(self.h, out.ctypes.data, 0, self.n), "dmxBatchDownloadBodyFlags")
        return out

    def idle_counters(self):
        """-> (steps_left [n] int32, time_left [n] float64)"""
        st, tl = np.zeros(self.n, np.int32), np.zeros(self.n, np.float64)
        _check(self.lib.dmxBatchIdleCounters(self.h, st.ctypes.data, tl.ctypes.data), "dmxBatchIdleCounters")
        return st, tl

    def auto_disable_stats(self):
        """asleep: slots asleep now; islands_skipped: in the last tick; slept / woken: bodies put to sleep by the rule / woken by
        the island rule since creation"""
        out = (C.c_int64 * 4)()
        _check(self.lib.dmxBatchAutoDisableStats(self.h, out), "dmxBatchAutoDisableStats")
        return dict(zip(AUTO_DISABLE_STATS, out))

    # -- damping, maximum angular speed, contact correction (include/dmx_batch.h, "damping"); step_joints only --
    def set_damping(self, lin_scale=0.0, ang_scale=0.0, lin_threshold=0.01, ang_threshold=0.01):
        """every slot's damping: velocities above the threshold are scaled by 1 - scale at the start of a tick"""
        _check(self.lib.dmxBatchSetDamping(self.h, float(lin_scale), float(ang_scale), float(lin_threshold), float(ang_threshold)),
               "dmxBatchSetDamping")

    def set_max_angular_speed(self, max_speed=float("inf")):
        """every slot's cap on |avel| (rad/s), applied by the integrator before the pose update"""
        _check(self.lib.dmxBatchSetMaxAngularSpeed(self.h, float(max_speed)), "dmxBatchSetMaxAngularSpeed")

    def upload_body_damping(self, table, first=0):
        """table: [k] BODY_DAMPING_DTYPE (or [k, 5] numbers in its field order) for slots first .. first + k - 1"""
        t = np.asarray(table)
        if t.dtype != BODY_DAMPING_DTYPE:
            t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 5).view(BODY_DAMPING_DTYPE).reshape(-1)
        t = np.ascontiguousarray(t)
        _check(self.lib.dmxBatchUploadBodyDamping(self.h, t.ctypes.data, int(first), t.shape[0]), "dmxBatchUploadBodyDamping")

    def body_damping(self):
        """-> [n] BODY_DAMPING_DTYPE (the defaults while no value has been set)"""
        out = np.zeros(self.n, BODY_DAMPING_DTYPE)
        _check(self.lib.dmxBatchDownloadBodyDamping(self.h, out.ctypes.data, 0, self.n), "dmxBatchDownloadBodyDamping")
        return out

    def set_contact_correction(self, surface_layer=0.0, max_correcting_vel=float("inf")):
        """depth the contacts may keep (m) and the cap on a contact's push-out velocity (m/s); a bounce may exceed the cap"""
        _check(self.lib.dmxBatchSetContactCorrection(self.h, float(surface_layer), float(max_correcting_vel)), "dmxBatchSetContactCorrection")

    def contact_correction(self):
        """-> (surface_layer, max_correcting_vel)"""
        a, b = C.c_double(), C.c_double()
        _check(self.lib.dmxBatchGetContactCorrection(self.h, C.byref(a), C.byref(b)), "dmxBatchGetContactCorrection")
        return a.value, b.value

    def set_row_order(self, order, seed=0):
        """ORDER_CREATION (default) / ORDER_ODE: the order QuickStep sweeps an island's rows in"""
        _check(self.lib.dmxBatchSetRowOrder(self.h, int(order), int(seed)), "dmxBatchSetRowOrder")

    def set_body_collisions(self, enable):
        _check(self.lib.dmxBatchSetBodyCollisions(self.h, int(enable)), "dmxBatchSetBodyCollisions")

    def collision_stats(self):
        out = (C.c_int64 * 6)()
        _check(self.lib.dmxBatchCollisionStats(self.h, out), "dmxBatchCollisionStats")
        d = dict(zip(("fast_ticks", "careful_ticks", "rebuilds", "pair_ticks", "last_pairs", "crowded"), out))
        ex = (C.c_int64 * 8)()
        _check(self.lib.dmxBatchCollisionStatsEx(self.h, ex), "dmxBatchCollisionStatsEx")
        d["unsupported_pairs"] = ex[6]
        d["speculated_ticks"] = ex[7]
        return d

    # -- the collision-checked loop in pieces (include/dmx_batch.h), for callers with per-tick work of their own --
    def chunk_begin(self):
        """-> (exact_only, ballistic)"""
        e, bl = C.c_int(), C.c_int()
        _check(self.lib.dmxBatchChunkBegin(self.h, C.byref(e), C.byref(bl)), "dmxBatchChunkBegin")
        return bool(e.value), bool(bl.value)

    def chunk_tick(self, h, check=True):
        _check(self.lib.dmxBatchChunkTick(self.h, h, int(check)), "dmxBatchChunkTick")

    def chunk_ticks(self, h, nticks, check_first=True, check_last=True):
        _check(self.lib.dmxBatchChunkTicks(self.h, h, nticks, int(check_first), int(check_last)), "dmxBatchChunkTicks")

    def set_snapshot_mode(self, mode):
        """SNAPSHOT_PINGPONG (default) / SNAPSHOT_COPY: how a chunk keeps its start state (include/dmx_batch.h)"""
        _check(self.lib.dmxBatchSetSnapshotMode(self.h, mode), "dmxBatchSetSnapshotMode")

    def set_exact_pipeline(self, mode):
        """EXACT_AUTO (default) / EXACT_STAGED / EXACT_ONE_WORKGROUP: how an exact tick runs its bookkeeping (include/dmx_batch.h)"""
        _check(self.lib.dmxBatchSetExactPipeline(self.h, mode), "dmxBatchSetExactPipeline")

    def set_class_pairs(self, class_a, class_b, enable):
        """whether bodies of two geometry classes collide with one another (the batch's form of ODE's category / collide bits)"""
        _check(self.lib.dmxBatchSetClassPairs(self.h, int(class_a), int(class_b), 1 if enable else 0), "dmxBatchSetClassPairs")

    def set_static_path(self, fused=True):
        """bodies at static boxes: the fused path (default) or the exact tick for every one of them (include/dmx_batch.h)"""
        _check(self.lib.dmxBatchSetStaticPath(self.h, 1 if fused else 0), "dmxBatchSetStaticPath")

    def set_ticks_per_launch(self, ticks):
        _check(self.lib.dmxBatchSetTicksPerLaunch(self.h, ticks), "dmxBatchSetTicksPerLaunch")

    def set_elision(self, mask):
        """bit 0: in-place launches of the contact-free tick store only what changed; bit 1: uniform mass / inertia travel as
        kernel arguments.  Default 3; 0 = every load and store (include/dmx_batch.h).  Same results bit for bit."""
        _check(self.lib.dmxBatchSetElision(self.h, int(mask)), "dmxBatchSetElision")

    def set_load_elision(self, on=True):
        """contact-free launches leave out the loads of pos.x/z and lvel.x/z in tiles that have proven them fixed (default on; active
        only while bit 0 of set_elision is on; include/dmx_batch.h).  Same results bit for bit."""
        _check(self.lib.dmxBatchSetLoadElision(self.h, 1 if on else 0), "dmxBatchSetLoadElision")

    def set_torque_free(self, on=True):
        """contact-free launches with uniform mass / inertia, no force accumulators and no gyroscopic torque take the short tick
        that builds no rotation matrix and no inverse inertia (default on; include/dmx_batch.h).  Same results bit for bit."""
        _check(self.lib.dmxBatchSetTorqueFree(self.h, 1 if on else 0), "dmxBatchSetTorqueFree")

    def torque_free_stats(self):
        """dict: contact-free launches that took a kernel with the short tick built in / the general kernel"""
        out = (C.c_int64 * 2)()
        _check(self.lib.dmxBatchTorqueFreeStats(self.h, out), "dmxBatchTorqueFreeStats")
        return {"short": int(out[0]), "general": int(out[1])}

    def set_lean_kernel(self, on=True):
        """lean contact-free launches with the short tick on run the straight-line kernel of their own (default on;
        include/dmx_batch.h).  Same results bit for bit."""
        _check(self.lib.dmxBatchSetLeanKernel(self.h, 1 if on else 0), "dmxBatchSetLeanKernel")

    def lean_kernel_stats(self):
        """dict: contact-free launches that took the straight-line kernel / any other kernel"""
        out = (C.c_int64 * 2)()
        _check(self.lib.dmxBatchLeanKernelStats(self.h, out), "dmxBatchLeanKernelStats")
        return {"lean_kernel": int(out[0]), "other": int(out[1])}

    def load_elision_stats(self):
        """dict: establish / lean launches, chain breaks, ended for good, tiles with x / z fixed.  Settles the batch."""
        out = (C.c_int64 * 6)()
        _check(self.lib.dmxBatchLoadElisionStats(self.h, out), "dmxBatchLoadElisionStats")
        keys = ("establish", "lean", "breaks", "ended", "tiles_x_fixed", "tiles_z_fixed")
        return {k: int(v) for k, v in zip(keys, out)}

    def check_zones_on(self, stream_handle, first, count):
        _check(self.lib.dmxBatchCheckZonesOnStream(self.h, stream_handle, first, count), "dmxBatchCheckZonesOnStream")

    def refresh_ghosts_on(self, stream_handle, first, count_lo, src_lo, count_hi, src_hi, check):
        _check(self.lib.dmxBatchRefreshGhostsOnStream(self.h, stream_handle, first, count_lo, src_lo, count_hi, src_hi, int(check)),
               "dmxBatchRefreshGhostsOnStream")

    def chunk_end(self):
        """-> (violated, warn); waits for the batch stream"""
        v, w = C.c_int(), C.c_int()
        _check(self.lib.dmxBatchChunkEnd(self.h, C.byref(v), C.byref(w)), "dmxBatchChunkEnd")
        return bool(v.value), bool(w.value)

    def chunk_commit(self, ticks, refresh_zones=False):
        _check(self.lib.dmxBatchChunkCommit(self.h, ticks, int(refresh_zones)), "dmxBatchChunkCommit")

    def chunk_rollback(self):
        _check(self.lib.dmxBatchChunkRollback(self.h), "dmxBatchChunkRollback")

    def exact_tick(self, h):
        _check(self.lib.dmxBatchExactTick(self.h, h), "dmxBatchExactTick")

    def find_pairs(self):
        """dSpaceCollide's pair search alone: -> (pairs [np, 2], involved [ni], cross [nc, 2] = (own body, ghost slot))"""
        pp, ip, cp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        npairs, ninv, nc = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.dmxBatchFindPairs(self.h, C.byref(pp), C.byref(npairs), C.byref(ip), C.byref(ninv)), "dmxBatchFindPairs")
        _check(self.lib.dmxBatchCrossPairs(self.h, C.byref(cp), C.byref(nc)), "dmxBatchCrossPairs")
        grab = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return (grab(pp, 2 * npairs.value).reshape(-1, 2), grab(ip, ninv.value), grab(cp, 2 * nc.value).reshape(-1, 2))

    # -- ray casts (include/dmx_batch.h) ----------------------------------------------------------------------------
    def ray_cast(self, origins, dirs, lengths, mask=RAY_ALL):
        """n rays (origins n x 3, dirs n x 3, lengths n) -> (ids int32 [n], hits [n, 7] = pos3 normal3 depth): per ray the first
        geom its segment crosses -- a body slot, RAY_PLANE, -3 - k for static box k, or RAY_MISS"""
        o = np.asarray(origins, dtype=self.dtype).reshape(-1, 3)
        n = o.shape[0]
        rays = np.empty((n, 7), self.dtype)
        rays[:, 0:3] = o
        rays[:, 3:6] = np.asarray(dirs, dtype=self.dtype).reshape(n, 3)
        rays[:, 6] = np.broadcast_to(np.asarray(lengths, dtype=self.dtype), (n,))
        ids = np.empty(n, np.int32)
        hits = np.empty((n, 7), self.dtype)
        _check(self.lib.dmxBatchRayCast(self.h, n, rays.ctypes.data if n else None, ids.ctypes.data if n else None,
                                        hits.ctypes.data if n else None, int(mask)), "dmxBatchRayCast")
        return ids, hits

    def ray_cast_device(self, rays_ptr, n, ids_ptr, hits_ptr, mask=RAY_ALL):
        """the same on device memory (n x 7 reals in, n int32 and n x 7 reals out; e.g. torch tensors' data_ptr()), enqueued on
        the batch's stream"""
        _check(self.lib.dmxBatchRayCastDevice(self.h, int(n), rays_ptr, ids_ptr, hits_ptr, int(mask)), "dmxBatchRayCastDevice")

    def set_ray_form(self, form):
        """RAY_FORM_AUTO (default: by the ray count) / RAY_FORM_LANE / RAY_FORM_WAVE / RAY_FORM_BRUTE; same results either way"""
        _check(self.lib.dmxBatchSetRayForm(self.h, int(form)), "dmxBatchSetRayForm")

    def set_active_count(self, n_active):
        _check(self.lib.dmxBatchSetActiveCount(self.h, n_active), "dmxBatchSetActiveCount")

    def step_range(self, h, first, count, reset_diag=False):
        _check(self.lib.dmxBatchStepRange(self.h, h, first, count, int(reset_diag)), "dmxBatchStepRange")

    def gather_bodies(self, idx_ptr, count, out_ptr):
        _check(self.lib.dmxBatchGatherBodies(self.h, idx_ptr, count, out_ptr), "dmxBatchGatherBodies")

    def scatter_bodies(self, idx_ptr, count, in_ptr):
        _check(self.lib.dmxBatchScatterBodies(self.h, idx_ptr, count, in_ptr), "dmxBatchScatterBodies")

    def scatter_bodies_on(self, stream_handle, idx_ptr, count, in_ptr):
        _check(self.lib.dmxBatchScatterBodiesOnStream(self.h, idx_ptr, count, in_ptr, stream_handle), "dmxBatchScatterBodiesOnStream")

    def set_boundary_pack(self, out_ptr, lo_count, hi_first):
        _check(self.lib.dmxBatchSetBoundaryPack(self.h, out_ptr, lo_count, hi_first), "dmxBatchSetBoundaryPack")

    def step_timed(self, h, nsteps):
        ms = C.c_float()
        _check(self.lib.dmxBatchStepTimed(self.h, h, nsteps, C.byref(ms)), "dmxBatchStepTimed")
        return ms.value

    def synchronize(self):
        _check(self.lib.dmxBatchSynchronize(self.h), "dmxBatchSynchronize")

    def set_stream(self, stream_handle):
        _check(self.lib.dmxBatchSetStream(self.h, stream_handle), "dmxBatchSetStream")

    def last_contact_count(self):
        n = C.c_int64()
        _check(self.lib.dmxBatchLastContactCount(self.h, C.byref(n)), "dmxBatchLastContactCount")
        return n.value

    def last_residual(self):
        r = C.c_double()
        _check(self.lib.dmxBatchLastResidual(self.h, C.byref(r)), "dmxBatchLastResidual")
        return r.value

    def transforms(self, first=0, count=None):
        count = self.n - first if count is None else count
        out = np.empty((count, 16), self.dtype)
        _check(self.lib.dmxBatchDownloadTransforms(self.h, out.ctypes.data, first, count),
               "dmxBatchDownloadTransforms")
        return out
