"""One tick of a constraint-free rigid body, restated in float64 from the definitions, with the populations, the comparability
rule, the condition model and the measured bands that tests/test_integrator_reference.py (CPU, through the two oracles) and
tests/test_gpu_integrator.py (every device copy of the integrator) hold the integrator to.  No tests in here.

Nothing below shares code with oracle/, csrc/ or tests/lcp_dense.py: rotations are 3 x 3 matrices built from the quaternion's
definition R(q) = 1 + 2 w [u]x + 2 [u]x^2, the inertia is R diag(I) R^T, the gyroscopic terms are evaluated in the body's principal
axes (the same equations, since R [a]x R^T = [R a]x, without the cancellations of the world-frame entries), the implicit update
is ONE linear solve (numpy.linalg.solve), and the quaternion product is written out once, from Hamilton's rules, in `_left_product`.  Which side the
angular velocity multiplies from is then TESTED, against rotation matrices (Rodrigues' formula, `rot`), not copied.

The tick (semi-implicit Euler, as ODE's dxStepBody after a step without constraints):
    f  = f_ext + m g                     v' = v + (h / m) f
    R  = R(q), I_w = R diag(I) R^T
    gyro off:       w' = w + h I_w^-1 t_ext
    gyro explicit:  w' = w + h I_w^-1 (t_ext - w x I_w w)
    gyro implicit:  w' = (I_w - h [I_w w]x)^-1 I_w w  +  h I_w^-1 t_ext
    x' = x + h v'                        q' = normalise(q + (h / 2) (0, w') (x) q)
f_ext and t_ext act in the tick after which they were set, and in no later one.  A quaternion is normalised when it is set
(dBodySetQuaternion); the zero quaternion becomes the identity.

DESIGN.md section 5, "float32 and float64 integration against the definition", carries the tables below and their derivation."""
import functools
from dataclasses import dataclass

import numpy as np

from __graft_entry__ import load_package

pkg = load_package()

H = 1.0 / 60.0
PITCH = 8.0
FAR = (4096.0, 0.0, -2560.0)                       # tests/pair_population.py's "far from the origin"
G = (0.0, -9.8, 0.0)
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
GYRO_OFF, GYRO_EXPLICIT, GYRO_IMPLICIT = 0, 1, 2
MODES = (GYRO_OFF, GYRO_EXPLICIT, GYRO_IMPLICIT)
MODE_NAME = {GYRO_OFF: "off", GYRO_EXPLICIT: "explicit", GYRO_IMPLICIT: "implicit"}
FIELDS = ("pos", "quat", "lvel", "avel")           # the order of Oracle.state() and BatchWorld.state()
N_GPU = 4133                                       # 2 x 2048 + 37: > 8 workgroups of 256, a partial workgroup, a partial wavefront
N_TICKS = 64
KAPPA_CLASSES = ("iso", "k3", "k30", "k1000")      # inertia ratio I_max / I_min: 1, (1, 3], (3, 30], (30, 1000]
_KAPPA_RANGE = {"k3": (1.0, 3.0), "k30": (3.0, 30.0), "k1000": (30.0, 1000.0)}
UNIFORM_INERTIA = {"k3": (0.5, 1.5, 0.875), "k30": (7.5, 0.25, 1.0), "k1000": (0.015625, 15.625, 0.25)}      # float32 values; kappa 3, 30, 1000
MAX_EXCUSED = 0.05                                 # a condition, not a measurement
ENERGY_GROWTH = 2.0                                # explicit gyro: excused when the float64 rotational energy grows beyond this


# ------------------------------------------------------------------------------------------------------------ the definition
def _cross_matrix(a):
    """[a]x, (n, 3) -> (n, 3, 3): [a]x b = a x b"""
    K = np.zeros(a.shape[:-1] + (3, 3))
    K[..., 0, 1] = -a[..., 2]; K[..., 0, 2] = a[..., 1]
    K[..., 1, 0] = a[..., 2]; K[..., 1, 2] = -a[..., 0]
    K[..., 2, 0] = -a[..., 1]; K[..., 2, 1] = a[..., 0]
    return K


def rot(axis, angle):
    """Rodrigues: the rotation by `angle` about the unit vector `axis`, 1 + sin(a) K + (1 - cos a) K^2"""
    K = _cross_matrix(np.asarray(axis, float))
    a = np.asarray(angle, float)[..., None, None]
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def rotation_of(q):
    """R(q) for q = (w, u): 1 + 2 w [u]x + 2 [u]x^2 -- for a unit q the rotation by 2 acos(w) about u / |u|"""
    q = np.asarray(q, float)
    K = _cross_matrix(q[..., 1:])
    return np.eye(3) + 2.0 * q[..., :1, None] * K + 2.0 * (K @ K)


def normalise(q):
    """q / |q|; the zero quaternion -> the identity"""
    q = np.asarray(q, float)
    l = np.linalg.norm(q, axis=-1, keepdims=True)
    one = np.zeros_like(q); one[..., 0] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(l > 0, q / np.where(l > 0, l, 1.0), one)


def _left_product(w, q):
    """(0, w) (x) q by Hamilton's rules (i^2 = j^2 = k^2 = ijk = -1): scalar -w.u, vector s w + w x u for q = (s, u)"""
    s, u = q[..., :1], q[..., 1:]
    return np.concatenate([-np.sum(w * u, axis=-1, keepdims=True), s * w + np.cross(w, u)], axis=-1)


def tick(state, mass, inertia, h, gravity, gyro, force=None, torque=None):
    """one tick of n free bodies in float64.  state = (pos, quat, lvel, avel); inertia (n, 3), the body-frame diagonal -> new state"""
    x, q, v, w = (np.asarray(a, float) for a in state)
    m = np.asarray(mass, float).reshape(-1, 1)
    Ib = np.asarray(inertia, float)
    f = m * np.asarray(gravity, float)[None, :] + (0.0 if force is None else np.asarray(force, float))
    t_ext = np.zeros_like(w) if torque is None else np.asarray(torque, float)
    with np.errstate(all="ignore"):
        v1 = v + (h / m) * f
        R = rotation_of(q)
        invIw = np.einsum("nij,nj,nkj->nik", R, 1.0 / Ib, R)
        push = h * np.einsum("nij,nj->ni", invIw, t_ext)
        # the gyroscopic part in the body's principal axes, where I_w = diag(I): the same equations (R [a]x R^T = [R a]x), free of
        # the cancellations of the world-frame entries, and exactly nothing for an isotropic body
        wb = np.einsum("nji,nj->ni", R, w)
        if gyro == GYRO_OFF:
            dwb = np.zeros_like(w)
        elif gyro == GYRO_EXPLICIT:                          # Euler's equations: (w x I w)_x = (I_z - I_y) w_y w_z, and cyclically
            c = np.stack([(Ib[:, 2] - Ib[:, 1]) * wb[:, 1] * wb[:, 2], (Ib[:, 0] - Ib[:, 2]) * wb[:, 2] * wb[:, 0],
                          (Ib[:, 1] - Ib[:, 0]) * wb[:, 0] * wb[:, 1]], axis=1)
            dwb = -h * c / Ib
        else:
            Lb = Ib * wb
            A = Ib[:, :, None] * np.eye(3) - h * _cross_matrix(Lb)
            ok = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(Lb).all(axis=1)
            dwb = np.full_like(w, np.nan)
            dwb[ok] = np.linalg.solve(A[ok], Lb[ok][..., None])[..., 0] - wb[ok]
        w1 = w + push + np.einsum("nij,nj->ni", R, dwb)
        x1 = x + h * v1
        q1 = normalise(q + 0.5 * h * _left_product(w1, q))
    return x1, q1, v1, w1


def rotational_energy(q, w, inertia):
    """1/2 w^T I_w w, in the body frame"""
    wb = np.einsum("nji,nj->ni", rotation_of(q), w)
    return 0.5 * np.sum(np.asarray(inertia, float) * wb * wb, axis=1)


# ------------------------------------------------------------------------------------------------------------ populations
@dataclass
class Population:
    """isolated bodies on an 8 m lattice: float64 arrays that hold float32 VALUES, so both precisions and the reference start from
    the same numbers.  mass (n,), inertia (n, 3), force / torque (n, 3) (zero rows: no call is made for them)."""
    name: str
    pos: np.ndarray
    quat: np.ndarray
    lvel: np.ndarray
    avel: np.ndarray
    mass: np.ndarray
    inertia: np.ndarray
    force: np.ndarray
    torque: np.ndarray
    kclass: np.ndarray          # index into KAPPA_CLASSES
    extreme: np.ndarray         # bool: the "extreme spin" class, |w| h in (0.5, 100]
    gravity: tuple
    far: bool

    @property
    def n(self):
        return len(self.pos)

    @property
    def place(self):
        return "far" if self.far else "near"

    @property
    def kappa(self):
        return self.inertia.max(axis=1) / self.inertia.min(axis=1)

    @property
    def forced(self):
        return self.force.any(axis=1) | self.torque.any(axis=1)

    @property
    def sides(self):
        return np.full((self.n, 3), 0.5)

    def start(self):
        """the state as the world holds it after the setters: the quaternion normalised (in float64)"""
        return self.pos, normalise(self.quat), self.lvel, self.avel

    def first(self, n):
        n = min(int(n), self.n)
        return Population(self.name, self.pos[:n], self.quat[:n], self.lvel[:n], self.avel[:n], self.mass[:n], self.inertia[:n],
                          self.force[:n], self.torque[:n], self.kclass[:n], self.extreme[:n], self.gravity, self.far)

    def without_forces(self):
        """the same bodies with no external force or torque on any of them"""
        z = np.zeros((self.n, 3))
        return Population(self.name + "-unforced", self.pos, self.quat, self.lvel, self.avel, self.mass, self.inertia, z, z, self.kclass,
                          self.extreme, self.gravity, self.far)

    def calm(self):
        """the same bodies with the horizontal velocity and force 1 / 32 of what they were: nobody leaves a broadphase safe zone (0.1 m
        on this lattice) within 64 ticks, so the collision proof's chunks are never rolled back"""
        s = np.array([1.0 / 32.0, 1.0, 1.0 / 32.0])
        return Population(self.name + "-calm", self.pos, self.quat, self.lvel * s, self.avel, self.mass, self.inertia, self.force * s,
                          self.torque, self.kclass, self.extreme, self.gravity, self.far)

    def uniform(self, cls, slow):
        """the same bodies with ONE mass and ONE anisotropic inertia of class `cls` for all of them (the batch then passes both as
        kernel arguments); forces and torques keep their accelerations.  slow: spin and torque scaled by a power of two <= 1 / (4 kappa),
        so that h kappa |w| stays below 0.02 and explicit gyro does not blow up within 64 ticks"""
        mass, inertia = 2.0, np.array(UNIFORM_INERTIA[cls])
        kap = inertia.max() / inertia.min()
        sc = 2.0 ** np.floor(np.log2(1.0 / (4.0 * kap))) if slow else 1.0
        n = self.n
        force = self.force * (mass / self.mass)[:, None]
        torque = self.torque * (inertia.min() / self.inertia.min(axis=1))[:, None] * sc
        return Population(f"{self.name}-uniform-{cls}", self.pos, self.quat, self.lvel, _f32(self.avel * sc), np.full(n, mass),
                          np.tile(inertia, (n, 1)), _f32(force), _f32(torque), np.full(n, KAPPA_CLASSES.index(cls)), self.extreme,
                          self.gravity, self.far)

    def scene(self, dtype, plane=None, static_boxes=None):
        n = self.n
        return pkg.scenes.Scene(self.pos, self.quat, self.lvel, self.avel, self.mass.reshape(n, 1), self.inertia, self.sides,
                                np.full(n, pkg.scenes.GEOM_BOX, np.uint8), plane, None, None, static_boxes).astype(dtype)

    def describe(self, i, h=H):
        """everything needed to rebuild body i alone"""
        i = int(i)
        return (f"body {i} of {self.name} ({self.place}, gravity {self.gravity}): class {KAPPA_CLASSES[int(self.kclass[i])]} "
                f"kappa={self.kappa[i]:.6g} |w|h={np.linalg.norm(self.avel[i]) * h:.6g}\n  pos={self.pos[i]!r} quat={self.quat[i]!r}\n"
                f"  lvel={self.lvel[i]!r} avel={self.avel[i]!r}\n  mass={self.mass[i]!r} inertia={self.inertia[i]!r}\n"
                f"  force={self.force[i]!r} torque={self.torque[i]!r}")


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _unit(rng, n, k=3):
    d = rng.normal(size=(n, k))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _draw(name, n, seed, classes, spin, extreme_every, gravity, far, h=H):
    """n bodies.  Body k: inertia class classes[k % len(classes)]; k % 3 == 0: an external force and torque; with extreme_every = 5,
    k % 5 == 4: extreme spin (4, 5 and 3 are coprime: every combination of class, spin regime and forcing occurs)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    kclass = np.array([KAPPA_CLASSES.index(c) for c in classes])[k % len(classes)]
    extreme = (k % extreme_every == extreme_every - 1) if extreme_every else np.zeros(n, bool)
    pos = np.stack([(k % 64) * PITCH, np.zeros(n), (k // 64) * PITCH], axis=1)
    if far:
        pos = pos + np.asarray(FAR)
    quat = _unit(rng, n, 4)
    inertia = np.empty((n, 3))
    scale = _logu(rng, 1e-2, 10.0, n)
    for c, cname in enumerate(KAPPA_CLASSES):
        m = np.flatnonzero(kclass == c)
        if cname == "iso":
            inertia[m] = 1.0
            continue
        lo, hi = _KAPPA_RANGE[cname]
        kap = _logu(rng, max(lo, 1.0 + 1e-3), hi, len(m))
        mid = _logu(rng, 1.0, kap, len(m))
        d = np.stack([np.ones(len(m)), mid, kap], axis=1)
        inertia[m] = np.take_along_axis(d, np.argsort(rng.random((len(m), 3)), axis=1), axis=1)      # any axis may be the slender one
    inertia *= scale[:, None]
    wh = np.where(extreme, _logu(rng, 0.5, 100.0, n), _logu(rng, spin[0], spin[1], n))
    avel = _unit(rng, n) * (wh / h)[:, None]
    mass = _logu(rng, 1e-3, 1e3, n)
    lvel = rng.uniform(-1.5, 1.5, (n, 3))
    forced = k % 3 == 0
    force = np.where(forced[:, None], mass[:, None] * rng.normal(size=(n, 3)) * 5.0, 0.0)
    torque = np.where(forced[:, None], (inertia.min(axis=1) * _logu(rng, 0.1, 100.0, n))[:, None] * _unit(rng, n), 0.0)
    inertia = _f32(inertia)
    iso = kclass == 0
    inertia[iso] = inertia[iso, :1]                                           # exactly isotropic after the rounding too
    return Population(name, _f32(pos), _f32(quat), _f32(lvel), _f32(avel), _f32(mass), inertia, _f32(force), _f32(torque),
                      kclass, extreme, tuple(gravity), bool(far))


VARIANTS = ("near", "far", "near0g")              # near the origin; translated by FAR; near the origin without gravity


@functools.lru_cache(maxsize=8)
def stress(variant="near", seed=101, n=N_GPU):
    """the ONE-TICK population: every inertia class, |w| h log-uniform in [1e-4, 0.5] and, every fifth body, in (0.5, 100]"""
    return _draw(f"stress[{variant},{seed}]", n, seed, KAPPA_CLASSES, (1e-4, 0.5), 5, (0.0, 0.0, 0.0) if variant == "near0g" else G,
                 variant == "far")


@functools.lru_cache(maxsize=8)
def flight(variant="near", seed=202, n=N_GPU):
    """the N-TICK population: classes iso and k3, |w| <= 3 rad/s (|w| h in [1e-4, 0.05]), no extreme spins -- the ranges in which the
    float64 reference itself stays stable over the run in every gyro mode (explicit gyro at kappa 30 and |w| = 3 does not)"""
    return _draw(f"flight[{variant},{seed}]", n, seed, ("iso", "k3"), (1e-4, 0.05), 0, (0.0, 0.0, 0.0) if variant == "near0g" else G,
                 variant == "far")


# ------------------------------------------------------------------------------------------------------------ the reference's runs
@functools.lru_cache(maxsize=64)
def reference_run(kind, variant, mode, ticks, seed=None, h=H, forced=True):
    """-> dict(state: the float64 reference after `ticks` ticks (read-only arrays), comparable: bool per body, decided from the
    reference ALONE: finite throughout, and -- explicit gyro -- the rotational energy never beyond ENERGY_GROWTH x the energy after
    the first tick (in which the external torque acts))"""
    pop = (stress if kind == "stress" else flight)(variant, *(() if seed is None else (seed,)))
    if not forced:
        pop = pop.without_forces()
    st = pop.start()
    ok = np.ones(pop.n, bool)
    e1 = None
    for t in range(ticks):
        st = tick(st, pop.mass, pop.inertia, h, pop.gravity, mode, pop.force if t == 0 else None, pop.torque if t == 0 else None)
        with np.errstate(all="ignore"):
            ok &= np.all([np.isfinite(a).all(axis=1) for a in st], axis=0)
            if mode == GYRO_EXPLICIT:
                e = rotational_energy(st[1], st[3], pop.inertia)
                if t == 0:
                    e1 = e
                ok &= np.isfinite(e) & (e <= ENERGY_GROWTH * e1)
    for a in st:
        a.setflags(write=False)
    ok.setflags(write=False)
    return dict(pop=pop, state=st, comparable=ok, excused=float(1.0 - ok.mean()))


# ------------------------------------------------------------------------------------------------------------ the condition model
def condition(pop, mode, h=H):
    """The magnitude each field's band is expressed in, per body: dict field -> (n, 3), (n, 1) or (n, 1).  DERIVED from the formulas
    of the tick as the product evaluates them (world frame, I_w = R diag(I) R^T formed entry by entry), not fitted:

    pos   per coordinate: |x_j| + h M_lvel            (the rounding of the sum, and h times the velocity's error)
    lvel  M_lvel = |v| + h (|f_ext| / m + |g|)        (the rounding of f_ext + m g, of (h / m) f and of the sum)
    avel  W = |w| + h |t_ext| / I_min                 (entries of I_w^-1 are sums of three terms of size 1 / I_min)
          off:       M = W
          explicit:  M = W + h kappa |w|^2            (I_w w carries eps I_max |w|; x w; h I_w^-1 multiplies by up to h / I_min)
          implicit:  M = W + kappa^2 |w| (1 + h|w|)   (below)
    quat  1 + (h / 2) M_avel                          (the rounding of a unit quaternion, and (h / 2) times w's error)

    Implicit mode is ODE's construction: t = (I_w Itild^-1 - 1) L / h with Itild = I_w - h [L]x, L = I_w w, and then w += h I_w^-1 t.
    The entries of the product I_w Itild^-1 are sums of three terms of size I_max / I_min = kappa that cancel to 1 + O(h |w| kappa):
    an absolute error of eps kappa, left standing by the "- 1".  It is multiplied by |L| / h <= I_max |w| / h and by h / I_min: eps
    kappa^2 |w|.  The true torque is of size kappa I_max |w|^2, and its rounding, through h / I_min, adds the factor (1 + h |w|)."""
    v = np.linalg.norm(pop.lvel, axis=1, keepdims=True)
    w = np.linalg.norm(pop.avel, axis=1, keepdims=True)
    m = pop.mass.reshape(-1, 1)
    imin = pop.inertia.min(axis=1, keepdims=True)
    kap = pop.kappa.reshape(-1, 1)
    aniso = (kap > 1.0).astype(float)                               # the product and the oracle skip the term for isotropic bodies
    m_lvel = v + h * (np.linalg.norm(pop.force, axis=1, keepdims=True) / m + float(np.linalg.norm(pop.gravity)))
    W = w + h * np.linalg.norm(pop.torque, axis=1, keepdims=True) / imin
    if mode == GYRO_OFF:
        m_avel = W
    elif mode == GYRO_EXPLICIT:
        m_avel = W + aniso * h * kap * w * w
    else:
        m_avel = W + aniso * kap * kap * w * (1.0 + h * w)
    return {"pos": np.abs(pop.pos) + h * m_lvel, "lvel": m_lvel, "avel": m_avel, "quat": 1.0 + 0.5 * h * m_avel}


def in_band_units(got, ref, pop, mode, eps, h=H):
    """per field: |got - ref| / (eps x condition model), (n,) -- the largest component of each body"""
    cond = condition(pop, mode, h)
    out = {}
    for name, a, b in zip(FIELDS, got, ref):
        with np.errstate(all="ignore"):
            out[name] = np.max(np.abs(np.asarray(a, float) - np.asarray(b, float)) / (eps * cond[name]), axis=1)
    return out


def n_tick_units(pop, mode, ticks=N_TICKS, h=H):
    """the units the N-tick deviations are reported in, from the START values: the one-tick magnitudes with the run's reach in them --
    pos: |x_j| + T (|v| + T |g|) + h M_lvel, T = ticks x h; lvel: M_lvel + T |g|; avel: M_avel; quat: 1"""
    c = condition(pop, mode, h)
    T = ticks * h
    g = float(np.linalg.norm(pop.gravity))
    v = np.linalg.norm(pop.lvel, axis=1, keepdims=True)
    return {"pos": np.abs(pop.pos) + T * (v + T * g) + h * c["lvel"], "lvel": c["lvel"] + T * g, "avel": c["avel"],
            "quat": np.ones((pop.n, 1))}


def n_tick_deviation(got, ref, pop, mode, ticks=N_TICKS, h=H):
    """per field: |got - ref| / (eps32 x n_tick_units), (n,)"""
    u = n_tick_units(pop, mode, ticks, h)
    with np.errstate(all="ignore"):
        return {name: np.max(np.abs(np.asarray(a, float) - np.asarray(b, float)) / (EPS32 * u[name]), axis=1)
                for name, a, b in zip(FIELDS, got, ref)}


# ------------------------------------------------------------------------------------------------------------ the oracle side
def oracle_run(pop, dtype, mode, ticks, h=H):
    """the population through the CPU oracle in `dtype`: bodies by the bulk adder, forces and torques by dBodyAddForce / AddTorque
    on the bodies that have one -> state after `ticks` ticks"""
    from oracle.orc_ctypes import Oracle                 # the code under test: only this runner and the measurements touch it
    orc = Oracle(dtype)
    ow = orc.world(gravity=pop.gravity)
    orc.lib.orc_world_set_gyro_mode(ow.w, int(mode))
    ow.add_boxes(pop.pos, pop.quat, pop.lvel, pop.avel, pop.mass, pop.inertia, pop.sides)
    for b in np.flatnonzero(pop.force.any(axis=1)):
        orc.lib.orc_body_add_force(ow.w, int(b), *[float(x) for x in pop.force[b]])
    for b in np.flatnonzero(pop.torque.any(axis=1)):
        orc.lib.orc_body_add_torque(ow.w, int(b), *[float(x) for x in pop.torque[b]])
    hh = orc.dtype.type(h)
    for _ in range(ticks):
        ow.tick(hh)
    assert ow.n_contacts() == 0
    st = ow.state()
    ow.close()
    return st


# ------------------------------------------------------------------------------------------------------------ the measured bands
# How every number below was fixed: `measure_one_tick` / `measure_n_ticks` at the bottom of this file, the
# oracle against the REFERENCE above, never against the code under test.
#
# ONE TICK.  The largest |oracle - reference| in units of eps x condition model over 25 seeds x 4 133 bodies (103 325) per gyro mode
# and place ("near" takes the larger of the with-gravity and the zero-gravity run), per field (pos, quat, lvel, avel):
ONE_TICK_MEASURED_F64 = {
    ('off', 'near'): (1.59, 1.5, 0.92, 6.66),
    ('off', 'far'): (1.56, 1.5, 0.914, 6.66),
    ('explicit', 'near'): (1.59, 2.15, 0.92, 6.66),
    ('explicit', 'far'): (1.56, 2.15, 0.914, 6.66),
    ('implicit', 'near'): (1.59, 1.5, 0.92, 15.7),
    ('implicit', 'far'): (1.56, 1.5, 0.914, 15.7),
}
ONE_TICK_MEASURED_F32 = {
    ('off', 'near'): (1.66, 1.24, 1.02, 10.3),
    ('off', 'far'): (1.66, 1.24, 1.02, 10.3),
    ('explicit', 'near'): (1.66, 2.68, 1.02, 10.3),
    ('explicit', 'far'): (1.66, 2.68, 1.02, 10.3),
    ('implicit', 'near'): (1.66, 1.24, 1.02, 10.3),
    ('implicit', 'far'): (1.66, 1.24, 1.02, 10.3),
}
# k (float32) and c (float64) of the bands k eps32 M and c eps64 M: 2 x the larger of the near and far maxima, rounded up to a
# power of two (the K_BAND rule), one per (field, gyro mode).
K_BAND = {
    ('pos', 'off'): 4, ('quat', 'off'): 4, ('lvel', 'off'): 4, ('avel', 'off'): 32,
    ('pos', 'explicit'): 4, ('quat', 'explicit'): 8, ('lvel', 'explicit'): 4, ('avel', 'explicit'): 32,
    ('pos', 'implicit'): 4, ('quat', 'implicit'): 4, ('lvel', 'implicit'): 4, ('avel', 'implicit'): 32,
}
C_BAND = {
    ('pos', 'off'): 4, ('quat', 'off'): 4, ('lvel', 'off'): 2, ('avel', 'off'): 16,
    ('pos', 'explicit'): 4, ('quat', 'explicit'): 8, ('lvel', 'explicit'): 2, ('avel', 'explicit'): 16,
    ('pos', 'implicit'): 4, ('quat', 'implicit'): 4, ('lvel', 'implicit'): 2, ('avel', 'implicit'): 32,
}

# The gyroscopic term ALONE: `avel` of the unforced anisotropic bodies (for them W = |w|, so the model is |w| plus the mode's gyroscopic
# term and nothing of the torque's), measured like the above, as (near, far) maxima per gyro mode; k and c by the same rule.  K_BAND's
# `avel` figure is set by the torque term and would hide a float32-only loss of the gyroscopic term by a factor of 30 - 300.
GYRO_MEASURED_F64 = {"explicit": (4.92, 4.92), "implicit": (1.07, 1.07)}
GYRO_MEASURED_F32 = {"explicit": (6.15, 6.15), "implicit": (0.999, 0.999)}
K_GYRO = {"explicit": 16, "implicit": 2}
C_GYRO = {"explicit": 16, "implicit": 4}

# N_TICKS ticks of `flight`: the largest |float32 oracle - reference| over the comparable bodies in eps32 x n_tick_units, per
# (inertia class, place, gyro mode), fields (pos, quat, lvel, avel).  The tolerance is TICK_FACTOR x these (the TICK_MEASURED rule:
# the margin covers the draw-to-draw spread of a maximum over 10^3 - 10^4 bodies).
TICK_MEASURED = {
    ('iso', 'near', 'off'): (31.6, 12.2, 5.01, 5.98),
    ('k3', 'near', 'off'): (31.6, 12.3, 5.09, 5.74),
    ('iso', 'far', 'off'): (31.7, 12.2, 5.01, 5.98),
    ('k3', 'far', 'off'): (31.6, 12.3, 5.09, 5.74),
    ('iso', 'near', 'explicit'): (31.6, 12.2, 5.01, 5.98),
    ('k3', 'near', 'explicit'): (31.6, 12.4, 5.09, 24.9),
    ('iso', 'far', 'explicit'): (31.7, 12.2, 5.01, 5.98),
    ('k3', 'far', 'explicit'): (31.6, 12.4, 5.09, 24.9),
    ('iso', 'near', 'implicit'): (31.6, 12.2, 5.01, 5.98),
    ('k3', 'near', 'implicit'): (31.6, 12.5, 5.09, 15.6),
    ('iso', 'far', 'implicit'): (31.7, 12.2, 5.01, 5.98),
    ('k3', 'far', 'implicit'): (31.6, 12.5, 5.09, 15.6),
}
TICK_FACTOR = 4.0


def one_tick_band(field, mode, dtype):
    """k (float32) or c (float64) for a field and gyro mode"""
    return (K_BAND if np.dtype(dtype).itemsize == 4 else C_BAND)[(field, MODE_NAME[mode])]


def n_tick_tolerance(cls, variant, mode):
    """{field: tolerance in eps32 x n_tick_units} for an inertia class ("iso" / "k3"), a variant and a gyro mode"""
    place = "far" if variant == "far" else "near"
    return {f: TICK_FACTOR * v for f, v in zip(FIELDS, TICK_MEASURED[(cls, place, MODE_NAME[mode])])}


# ------------------------------------------------------------------------------------------------------------ the checks
def finite_rows(state):
    return np.all([np.isfinite(np.asarray(a, float)).all(axis=1) for a in state], axis=0)


def _worst(dev, mask, pop, bound, what, unit):
    """the largest deviation per field over `mask`; AssertionError naming the worst body of the first field over its bound"""
    out = {}
    for f in FIELDS:
        d = np.where(mask, dev[f], 0.0)
        d = np.where(np.isnan(d), np.inf, d)
        i = int(np.argmax(d))
        out[f] = float(d[i])
        assert d[i] <= bound[f], (f"{what}: {f} deviates by {d[i]:.4g} {unit}, bound {bound[f]:.4g}\n" + pop.describe(i))
    return out


def check_one_tick(got, ref, pop, mode, dtype, what, h=H):
    """`got` (a state in `dtype`) against `ref` after ONE tick of `pop`: wherever ref is finite, got is finite and within
    k eps M (float32) / c eps M (float64) of it.  -> {field: the largest deviation in eps x condition model}"""
    fin = finite_rows(ref)
    bad = fin & ~finite_rows(got)
    assert not bad.any(), f"{what}: not finite where the reference is\n" + pop.describe(np.flatnonzero(bad)[0])
    eps = EPS32 if np.dtype(dtype).itemsize == 4 else EPS64
    bound = {f: one_tick_band(f, mode, dtype) for f in FIELDS}
    dev = in_band_units(got, ref, pop, mode, eps, h)
    unit = f"{'eps32' if eps == EPS32 else 'eps64'} x model"
    out = _worst(dev, fin, pop, bound, f"{what} [{MODE_NAME[mode]}, {np.dtype(dtype).name}, 1 tick]", unit)
    if mode != GYRO_OFF:
        m = gyro_alone(pop) & fin
        kg = (K_GYRO if eps == EPS32 else C_GYRO)[MODE_NAME[mode]]
        i = int(np.argmax(np.where(m, dev["avel"], 0.0)))
        out["gyro"] = float(dev["avel"][i]) if m.any() else 0.0
        assert out["gyro"] <= kg, (f"{what} [{MODE_NAME[mode]}, {np.dtype(dtype).name}, 1 tick]: avel of an unforced body (the gyroscopic term "
                                   f"alone) deviates by {out['gyro']:.4g} {unit}, bound {kg}\n" + pop.describe(i))
    return out


def gyro_alone(pop):
    """the bodies whose `avel` model holds the gyroscopic term and |w| only: anisotropic, no torque"""
    return (pop.kappa > 1.0) & ~pop.torque.any(axis=1)


def check_n_ticks(got, ref, comparable, pop, variant, mode, what, ticks=N_TICKS, h=H):
    """a float32 state against a float64 one after `ticks` ticks of the flight population, on the comparable bodies, per inertia
    class.  -> {class: {field: the largest deviation in eps32 x n_tick_units}}"""
    bad = comparable & ~finite_rows(got)
    assert not bad.any(), f"{what}: not finite where the reference is\n" + pop.describe(np.flatnonzero(bad)[0])
    dev = n_tick_deviation(got, ref, pop, mode, ticks, h)
    out = {}
    for c in sorted(set(pop.kclass.tolist())):
        cls = KAPPA_CLASSES[c]
        out[cls] = _worst(dev, comparable & (pop.kclass == c), pop, n_tick_tolerance(cls, variant, mode),
                          f"{what} [{MODE_NAME[mode]}, {cls}, {variant}, {ticks} ticks]", "eps32 x n-tick units")
    return out


def check_unit_quaternions(quat, ok, pop, what, ulps=4):
    q = np.asarray(quat)
    eps = EPS32 if q.dtype.itemsize == 4 else EPS64
    err = np.abs(np.linalg.norm(q.astype(float), axis=1) - 1.0)
    err = np.where(ok, err, 0.0)
    i = int(np.argmax(err))
    assert err[i] <= ulps * eps, f"{what}: |q| - 1 = {err[i] / eps:.3g} eps, bound {ulps}\n" + pop.describe(i)
    return float(err[i] / eps)


# ------------------------------------------------------------------------------------------------------------ the measurement
def _pow2_at_least(x):
    return float(2.0 ** np.ceil(np.log2(x)))


def measure_one_tick(seeds=range(25), n=N_GPU):
    """-> (float64 maxima, float32 maxima), each {(mode name, place): (pos, quat, lvel, avel)}, and the same two for `avel` of
    the `gyro_alone` bodies, {(mode name, place): maximum}"""
    out = {"float64": {}, "float32": {}}
    gyro = {"float64": {}, "float32": {}}
    for mode in MODES:
        for variant in VARIANTS:
            place = "far" if variant == "far" else "near"
            for seed in seeds:
                ref = reference_run("stress", variant, mode, 1, seed=1000 + seed)
                pop, fin = ref["pop"], np.all([np.isfinite(a).all(axis=1) for a in ref["state"]], axis=0)
                for dtype, eps in (("float64", EPS64), ("float32", EPS32)):
                    dev = in_band_units(oracle_run(pop, dtype, mode, 1), ref["state"], pop, mode, eps)
                    worst = tuple(float(np.max(dev[f][fin])) for f in FIELDS)
                    key = (MODE_NAME[mode], place)
                    out[dtype][key] = tuple(max(a, b) for a, b in zip(out[dtype].get(key, (0.0,) * 4), worst))
                    if mode != GYRO_OFF:
                        g = float(np.max(dev["avel"][fin & gyro_alone(pop)]))
                        gyro[dtype][key] = max(gyro[dtype].get(key, 0.0), g)
    return out["float64"], out["float32"], gyro["float64"], gyro["float32"]


def measure_n_ticks(ticks=N_TICKS):
    out = {}
    for mode in MODES:
        for variant in VARIANTS:
            place = "far" if variant == "far" else "near"
            ref = reference_run("flight", variant, mode, ticks)
            pop = ref["pop"]
            dev = n_tick_deviation(oracle_run(pop, "float32", mode, ticks), ref["state"], pop, mode, ticks)
            for c in (0, 1):
                m = ref["comparable"] & (pop.kclass == c)
                key = (KAPPA_CLASSES[c], place, MODE_NAME[mode])
                worst = tuple(float(np.max(dev[f][m])) for f in FIELDS)
                out[key] = tuple(max(a, b) for a, b in zip(out.get(key, (0.0,) * 4), worst))
    return out


def measure_kappa_table(n=1000, seed=7, h=H):
    """the float32 oracle against the reference after ONE tick of n unforced bodies with body inertia a permutation of (1, u, kappa),
    u log-uniform in [1, kappa], at |w| = 0.1, 3 and 30 rad/s: {(mode name, kappa): [(|w|, max |d avel| / (eps32 |w|), max |d quat| /
    eps32)]} -- DESIGN.md's per-mode, per-kappa table"""
    out = {}
    for mode in MODES:
        for kap in (1.0, 3.0, 30.0, 1000.0):
            rows = []
            for wn in (0.1, 3.0, 30.0):
                rng = np.random.default_rng(seed)
                d = np.stack([np.ones(n), _logu(rng, 1.0, kap, n) if kap > 1 else np.ones(n), np.full(n, kap)], axis=1)
                inertia = _f32(np.take_along_axis(d, np.argsort(rng.random((n, 3)), axis=1), axis=1))
                k = np.arange(n)
                pos = np.stack([(k % 64) * PITCH, np.zeros(n), (k // 64) * PITCH], axis=1)
                z = np.zeros((n, 3))
                pop = Population(f"kappa{kap:g}", _f32(pos), _f32(_unit(rng, n, 4)), z, _f32(_unit(rng, n) * wn), np.ones(n), inertia, z, z,
                                 np.zeros(n, int), np.zeros(n, bool), (0.0, 0.0, 0.0), False)
                ref = tick(pop.start(), pop.mass, pop.inertia, h, pop.gravity, mode)
                got = oracle_run(pop, "float32", mode, 1, h)
                da = np.max(np.abs(got[3].astype(float) - ref[3])) / (EPS32 * wn)
                dq = np.max(np.abs(got[1].astype(float) - ref[1])) / EPS32
                rows.append((wn, float(da), float(dq)))
            out[(MODE_NAME[mode], kap)] = rows
    return out


if __name__ == "__main__":                         # python -m tests.integrator_reference: prints the tables above, freshly measured
    m64, m32, g64, g32 = measure_one_tick()
    fmt = lambda d: "{\n" + "".join(f"    {k!r}: ({', '.join(f'{v:.3g}' for v in vals)}),\n" for k, vals in d.items()) + "}"
    print("ONE_TICK_MEASURED_F64 =", fmt(m64))
    print("ONE_TICK_MEASURED_F32 =", fmt(m32))
    for name, m in (("C_BAND", m64), ("K_BAND", m32)):
        band = {(f, MODE_NAME[mode]): _pow2_at_least(2.0 * max(m[(MODE_NAME[mode], p)][i] for p in ("near", "far")))
                for mode in MODES for i, f in enumerate(FIELDS)}
        print(name, "=", band)
    for name, g in (("GYRO_MEASURED_F64", g64), ("GYRO_MEASURED_F32", g32)):
        print(name, "=", {m: tuple(round(g[(m, p)], 3) for p in ("near", "far")) for m in ("explicit", "implicit")})
    for name, g in (("C_GYRO", g64), ("K_GYRO", g32)):
        print(name, "=", {m: _pow2_at_least(2.0 * max(g[(m, p)] for p in ("near", "far"))) for m in ("explicit", "implicit")})
    print("TICK_MEASURED =", fmt(measure_n_ticks()))
    for key, rows in measure_kappa_table().items():
        print(key, " ".join(f"|w|={w:g}: avel {a:.3g} quat {q:.3g};" for w, a, q in rows))
