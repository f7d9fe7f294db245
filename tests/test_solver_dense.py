"""The dense float64 reference of the contact solver (tests/lcp_dense.py) pinned by algebra and known answers, and the CPU
oracle's two steppers (oracle/orc_step.c) pinned by the reference.  The oracle and the HIP kernels were written by the same
hand; the reference is a second route from the definitions (include/dmx_batch.h), so a mistake
shared by the first two shows up here.  CPU only."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lcp_dense as ld
import quick_band as qb
from __graft_entry__ import load_package

H = 1.0 / 60.0
G = 9.8


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rand_quat(rng):
    return _unit(rng.normal(size=4))


def _bodies(n, rng, spread=1.0, aniso=True, speed=0.3):
    pos = rng.uniform(-spread, spread, (n, 3))
    quat = np.array([_rand_quat(rng) for _ in range(n)])
    lvel = rng.normal(scale=speed, size=(n, 3))
    avel = rng.normal(scale=speed, size=(n, 3))
    mass = rng.uniform(0.5, 2.0, n)
    inertia = rng.uniform(0.2, 1.0, (n, 3)) if aniso else np.ones((n, 3))
    return ld.Bodies(pos, quat, lvel, avel, mass, inertia)


def _contacts(bodies, pairs, rng, per=3, mu=np.inf, mode=ld.CONTACT_BOUNCE, bounce=0.2, bounce_vel=0.1):
    """synthetic contacts: for each (b1, b2) `per` contacts at points within 0.6 of b1's centre, normals pointing roughly
    from b2 (or from below, for static) into b1, depths in [0, 0.05]"""
    out = []
    for b1, b2 in pairs:
        axis = bodies.pos[b1] - bodies.pos[b2] if b2 >= 0 else np.array([0.0, 1.0, 0.0])
        axis = _unit(axis + 1e-9)
        for _ in range(per):
            n = _unit(axis + 0.4 * rng.normal(size=3))
            p = bodies.pos[b1] + 0.6 * _unit(rng.normal(size=3)) * rng.uniform(0.2, 1.0)
            out.append((p, n, rng.uniform(0, 0.05), b1, b2, mode, mu, bounce, bounce_vel, 0.0, 0.0))
    return np.array(out, ld.JOINT_DTYPE)


# ---------------------------------------------------------------------------------------------------------------------
# the reference against itself
@pytest.mark.parametrize("n", [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0.6, 0.0, 0.8), (0.0, 0.70710679, 0.70710677),
                               (0.0, 0.70710677, 0.70710679), (-0.3, 0.5, -0.81)])
def test_plane_space_is_a_right_handed_orthonormal_frame(n):
    n = _unit(n)
    t1, t2 = ld.plane_space(n)
    F = np.array([t1, t2, n])
    assert np.max(np.abs(F @ F.T - np.eye(3))) < 1e-15
    assert np.max(np.abs(np.cross(t1, t2) - n)) < 1e-15
    # the branch: t1 lies in the yz plane when |n_z| > 1/sqrt(2), in the xy plane otherwise
    assert (t1[0] == 0.0) if abs(n[2]) > np.sqrt(0.5) else (t1[2] == 0.0)


def _literal_ode_sor(I, iters, w):
    """dxQuickStepper's SOR_LCP as ODE writes it (SURVEY a-7): per row iMJ = M^-1 J^T, Ad = w / (J iMJ + cfm/h), rows and
    rhs scaled by Ad, the body accumulator a = M^-1 J^T lambda updated row by row"""
    m = I.m
    cfm = I.cfm / I.h
    iMJ = I.Minv @ I.J.T                      # 6nb x m
    Ad = np.array([w / (I.J[i] @ iMJ[:, i] + cfm[i]) for i in range(m)])
    Js = I.J * Ad[:, None]
    rhs = I.b * Ad
    Adcfm = Ad * cfm
    lam = np.zeros(m)
    a = np.zeros(I.J.shape[1])
    for _ in range(iters):
        for i in range(m):
            delta = rhs[i] - lam[i] * Adcfm[i] - Js[i] @ a
            new = min(max(lam[i] + delta, I.lo[i]), I.hi[i])
            a += iMJ[:, i] * (new - lam[i])
            lam[i] = new
    return lam


def _island(seed, mu, n=4, per=3, gyro=ld.GYRO_OFF):
    rng = np.random.default_rng(seed)
    B = _bodies(n, rng)
    pairs = [(k, k - 1) for k in range(1, n)] + [(0, -1)]
    jts = _contacts(B, pairs, rng, per=per, mu=mu)
    W = ld.World(gyro=gyro, cfm=1e-5)
    (slots, cj), = ld.islands(B, ld.canonical(B, jts))
    return B, W, jts, ld.Island(B, W, slots, cj, jts)


@pytest.mark.parametrize("mu", [0.0, 0.4, np.inf])
def test_dense_pgs_equals_odes_accumulator_form(mu):
    """the dense update lambda_i += w (b_i - (A lambda)_i) / A_ii is ODE's Ad / iMJ form rewritten: same numbers to 1e-14"""
    _, W, _, I = _island(1, mu)
    got, _ = I.quickstep(W.iters, W.sor_w)
    want = _literal_ode_sor(I, W.iters, W.sor_w)
    assert np.max(np.abs(got - want)) <= 1e-14 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("mu", [0.0, 0.4, np.inf])
def test_quickstep_converges_to_the_exact_solution(mu):
    """SOR's fixed point is the LCP's solution (A is positive definite): 20 000 sweeps reach exact()'s velocities (lambda
    itself is ill-conditioned along redundant contacts, the velocities it makes are not)"""
    _, _, _, I = _island(2, mu, n=3, per=1)
    ex, info = I.exact()
    qs, _ = I.quickstep(20000, 1.0)
    v_ex, v_qs = I.velocities(ex), I.velocities(qs)
    assert np.max(np.abs(v_qs - v_ex)) <= 1e-8 * max(G * H, np.max(np.abs(v_ex)))


@pytest.mark.parametrize("mu", [0.0, 0.4, np.inf])
def test_exact_does_not_depend_on_the_row_order(mu):
    """the LCP's solution is unique: permuting the rows permutes lambda and nothing else"""
    _, _, _, I = _island(3, mu)
    lam, _ = I.exact()
    p = np.random.default_rng(0).permutation(I.m)
    I.A, I.b, I.lo, I.hi = I.A[np.ix_(p, p)], I.b[p], I.lo[p], I.hi[p]
    lam_p, _ = I.exact()
    assert np.max(np.abs(lam_p - lam[p])) <= 1e-9 * max(1.0, np.max(np.abs(lam)))


def test_exact_rejects_an_answer_that_breaks_complementarity():
    """the certificate is a real check: a lambda nudged off the solution fails it"""
    _, _, _, I = _island(4, 0.4)
    lam, _ = I.exact()
    state = np.full(I.m, ld.FREE)
    with pytest.raises(ld.ReferenceError):
        I.certify(lam + 1e-3, state)


def _box_stack(n, mu=np.inf, vx=0.0):
    """n unit boxes (m = 1, I = 1) stacked on static ground at rest, four corner contacts per interface, depth 0"""
    B = ld.Bodies([[0, 0.5 + k, 0] for k in range(n)], [[1, 0, 0, 0]] * n, [[vx, 0, 0]] * n, np.zeros((n, 3)),
                  np.ones(n), np.ones((n, 3)))
    out = []
    for k in range(n):
        for dx, dz in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
            out.append(((dx, float(k), dz), (0, 1, 0), 0.0, k, k - 1 if k else -1, 0, mu, 0, 0, 0, 0))
    return B, np.array(out, ld.JOINT_DTYPE)


def test_known_answer_three_box_stack_carries_3mg_2mg_mg():
    B, jts = _box_stack(3)
    W = ld.World(erp=0.0, cfm=1e-10)
    r = ld.step(B, W, jts, "exact")
    lam = r.normal_lambda(len(jts)).reshape(3, 4).sum(axis=1)
    assert np.max(np.abs(lam - np.array([3, 2, 1]) * G)) < 1e-6
    assert np.max(np.abs(r.bodies.lvel)) < 1e-8


@pytest.mark.parametrize("vx", [3.0, -3.0])
def test_known_answer_sliding_box_friction_saturates_at_mu(vx):
    """a box sliding along x: the friction rows along x (dPlaneSpace's t1 = -x for n = +y) end at +-mu -- ODE's friction
    box is a force bound, not mu times the normal force -- and the ones along z carry nothing"""
    mu = 0.5
    B, jts = _box_stack(1, mu=mu, vx=vx)
    W = ld.World(erp=0.0)
    r = ld.step(B, W, jts, "exact")
    (I,), (lam,), (info,) = r.islands, r.lams, r.infos
    t1 = lam[I.row_kind == 1]
    assert np.allclose(t1, mu if vx > 0 else -mu, rtol=0, atol=1e-12)
    assert np.max(np.abs(lam[I.row_kind == 2])) < 1e-9
    assert (info["n_hi"], info["n_lo"]) == ((4, 0) if vx > 0 else (0, 4))
    assert abs(r.bodies.lvel[0, 0] - (vx - np.sign(vx) * 4 * mu * H)) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
def _oracle_world(orc, kind, seed):
    """-> (oracle world, masses, inertias, flags) of one scene; the bodies are created in slot order"""
    rng = np.random.default_rng(seed)
    w = orc.world()
    w.add_plane(0, 1, 0, 0)
    if kind in ("stack3", "column12"):
        n = 3 if kind == "stack3" else 12
        pos = np.array([[0.0, 0.5 + 0.999 * k, 0.0] for k in range(n)])
        quat = np.tile([1.0, 0, 0, 0], (n, 1))
        lv = np.zeros((n, 3)); lv[:, 1] = -0.2; lv[:, 0] = 0.01 * np.arange(n)
        av = np.zeros((n, 3))
        mass, inertia = np.ones(n), np.ones((n, 3))
        w.add_boxes(pos, quat, lv, av, mass, inertia, np.ones((n, 3)))
    elif kind in ("pile_boxes", "pile_spheres"):
        n = 10 if kind == "pile_boxes" else 24
        pos = np.column_stack([rng.uniform(-0.8, 0.8, n), 0.45 + 0.55 * np.arange(n) / 2.5, rng.uniform(-0.8, 0.8, n)])
        quat = np.array([_rand_quat(rng) for _ in range(n)])
        lv = rng.normal(scale=0.5, size=(n, 3)); av = rng.normal(scale=1.0, size=(n, 3))
        mass = rng.uniform(0.5, 2.0, n); inertia = rng.uniform(0.1, 0.6, (n, 3))
        if kind == "pile_boxes":
            w.add_boxes(pos, quat, lv, av, mass, inertia, rng.uniform(0.6, 1.0, (n, 3)))
        else:
            w.add_spheres(pos, quat, lv, av, mass, inertia, rng.uniform(0.4, 0.6, (n, 1)))
    else:                                                          # a sphere resting on two boxes
        pos = np.array([[-0.5, 0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 1.35, 0.0]])
        quat = np.tile([1.0, 0, 0, 0], (3, 1))
        lv = np.zeros((3, 3)); lv[2, 1] = -0.5
        av = np.zeros((3, 3)); av[2] = (0.3, 0.0, 0.2)
        mass, inertia = np.array([1.0, 1.5, 0.7]), np.array([[0.2, 0.3, 0.4], [0.3, 0.3, 0.5], [0.1, 0.2, 0.15]])
        w.add_boxes(pos[:2], quat[:2], lv[:2], av[:2], mass[:2], inertia[:2], np.ones((2, 3)))
        w.add_spheres(pos[2:], quat[2:], lv[2:], av[2:], mass[2:], inertia[2:], [[0.5]])
    return w, mass, inertia


SCENES = ["stack3", "column12", "pile_boxes", "pile_spheres", "sphere_on_boxes"]


@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("gyro", [ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT])
@pytest.mark.parametrize("bounce", [False, True])
@pytest.mark.parametrize("mu", [0.0, 0.3, np.inf])
@pytest.mark.parametrize("scene", SCENES)
def test_oracle_tick_equals_the_dense_reference(orc64, scene, mu, bounce, gyro, stepper):
    """one oracle tick rebuilt in numpy from the oracle's pre-tick state and its contact joints (World.joints(): bodies and
    normal already canonical).  Tolerances (float64, both sides solve the same system): QuickStep -- the same sweeps in
    the same order, only the summation order differs -- 1e-12 on velocities relative to max(|v|, g h) and 1e-10 relative on
    the normal lambdas; dWorldStep -- two different exact methods on an A with cfm / h = 6e-9 on its diagonal -- 1e-9.
    The pile of boxes runs at cfm 1e-5: at 1e-10 its A (up to eight contacts per overlapping pair) has kappa ~ 1e9 and
    not even the reference's solve certifies.  Regression: with friction that pile made the oracle's exact solve cycle
    to its round limit (block flips undoing Murty's single flips, oracle/orc_step.c exact_lcp)."""
    cfm = 1e-5 if scene == "pile_boxes" else 1e-10
    w, mass, inertia = _oracle_world(orc64, scene, seed=7)
    orc64.lib.orc_world_set_cfm(w.w, cfm)
    mode = ld.CONTACT_BOUNCE if bounce else 0
    orc64.lib.orc_world_set_surface(w.w, mode, mu, 0.2, 0.1)
    orc64.lib.orc_world_set_gyro_mode(w.w, gyro)
    w.set_stepper(stepper == "exact")
    pos, quat, lv, av = w.state()
    w.tick(H)
    after = w.state()
    if stepper == "exact":
        m = sum(3 if mu > 0 else 1 for _ in w.joints())
        assert orc64.lib.orc_world_last_lcp_rounds(w.w) < 20 * m + 100, "the oracle's exact solve ran out of rounds"
    raw = w.joints()
    assert raw, "the scene makes no contacts"
    jts = np.array([(p, n, d, b1, b2, mode, mu, 0.2, 0.1, 0.0, 0.0) for b1, b2, p, n, d, _ in raw], ld.JOINT_DTYPE)
    B = ld.Bodies(pos, quat, lv, av, mass, inertia)
    W = ld.World(h=H, erp=0.2, cfm=cfm, gyro=gyro)
    r = ld.step(B, W, jts, stepper)
    scale = ld.velocity_scale(r.bodies, W)
    tol = 1e-12 if stepper == "quick" else 1e-9
    assert ld.velocity_error(r.bodies, after[2], after[3]) <= tol * scale
    assert np.max(np.abs(after[0] - r.bodies.pos)) <= tol * scale * H + 1e-15
    if stepper == "quick":
        # (dWorldStep's lambdas are not compared: four coplanar contacts per face make A's condition number ~1e9, so the
        # split of a face's load between its contacts is fixed only to ~1e-7 by either solver; the velocities are not)
        lam_ref = r.normal_lambda(len(jts))
        lam_orc = np.array([x[5] for x in raw])
        assert np.max(np.abs(lam_orc - lam_ref)) <= 1e-10 * max(1.0, np.max(np.abs(lam_ref)))


@functools.lru_cache(maxsize=None)
def oracle_tick_f32(orc, scene, mu, bounce, gyro):
    """one QuickStep tick of the float32 oracle at cfm 1e-5 and the reference built from the oracle's own float32 pre-tick
    state, world parameters and joints (as tests/test_gpu_solver_dense.py as_precision does for a float32 batch).
    -> (reference Result, World, oracle's post-tick state (n, 13), oracle's normal lambdas, joints); shared, unchanged,
    by every test that needs it (tests/test_quick_band.py measures the band's K on these)"""
    r32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    w, mass, inertia = _oracle_world(orc, scene, seed=7)
    orc.lib.orc_world_set_cfm(w.w, 1e-5)
    mode = ld.CONTACT_BOUNCE if bounce else 0
    orc.lib.orc_world_set_surface(w.w, mode, mu, 0.2, 0.1)
    orc.lib.orc_world_set_gyro_mode(w.w, gyro)
    w.set_stepper(False)
    pos, quat, lv, av = [np.asarray(x, np.float64) for x in w.state()]
    w.tick(H)
    post = np.column_stack([np.asarray(x, np.float64) for x in w.state()])
    raw = w.joints()
    w.close()
    assert raw, "the scene makes no contacts"
    jts = np.array([(p, n, d, b1, b2, mode, float(r32(mu)), float(r32(0.2)), float(r32(0.1)), 0.0, 0.0)
                    for b1, b2, p, n, d, _ in raw], ld.JOINT_DTYPE)
    B = ld.Bodies(pos, quat, lv, av, r32(mass), r32(inertia))
    W = ld.World(h=float(r32(H)), gravity=r32([0.0, -9.8, 0.0]), erp=float(r32(0.2)), cfm=float(r32(1e-5)),
                 sor_w=float(r32(1.3)), gyro=gyro)
    return ld.step(B, W, jts, "quick"), W, post, np.array([x[5] for x in raw], np.float64), jts


@pytest.mark.parametrize("gyro", [ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT])
@pytest.mark.parametrize("bounce", [False, True])
@pytest.mark.parametrize("mu", [0.0, 0.3, np.inf])
@pytest.mark.parametrize("scene", SCENES)
def test_oracle_tick_equals_the_dense_reference_f32(orc32, scene, mu, bounce, gyro):
    """the float32 oracle's QuickStep -- the arithmetic of every float32 kernel that collides for itself, bit for bit -- against
    the float64 reference, clamps included: velocities, positions and quaternions per body within the band of
    tests/quick_band.py (K eps32 M_v; no clamp-margin gate), and the normal lambda within K eps32 max |lambda| on the rows
    whose own reference margin is above 1e-3 of the island's largest |lambda| (a row that sits at its bound may differ by a
    flip; velocities may not)."""
    r, W, post, lam_orc, jts = oracle_tick_f32(orc32, scene, mu, bounce, gyro)
    K = qb.K["contact"]
    worst = qb.assert_in_band(r, W, post, K, what=f"float32 oracle {scene}")
    print(f"f32 oracle {scene} mu={mu} bounce={bounce} gyro={gyro}: {worst:.2f} eps32 M_v (K = {K})")
    for I, lam in zip(r.islands, r.lams):
        if not I.m:
            continue
        _, margins = qb.row_margins(I, W.iters, W.sor_w)
        top = np.max(np.abs(lam))
        ok = (I.row_kind == 0) & (margins > 1e-3 * top)
        d = np.abs(lam_orc[I.row_joint[ok]] - lam[ok])
        assert np.all(d <= K * qb.EPS32 * top), f"normal lambda off by {d.max() / (qb.EPS32 * top):.2f} eps32 max|lambda|"


# ---------------------------------------------------------------------------------------------------------------------
def test_contact_joint_dtype_matches_the_c_layout(tmp_path):
    """batch.CONTACT_JOINT_DTYPE is dmxContactJoint as a C compiler lays it out (include/dmx_batch.h): every field's offset
    and the struct's size, printed by a program compiled against the header"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "joint_layout.c"
    fields = ["pos", "normal", "depth", "body1", "body2", "mode", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"dmx_batch.h\"\nint main(void) {\n" +
                   "".join(f'    printf("{f} %zu\\n", offsetof(dmxContactJoint, {f}));\n' for f in fields) +
                   '    printf("sizeof %zu\\n", sizeof(dmxContactJoint));\n    return 0;\n}\n')
    exe = str(tmp_path / "joint_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", exe],
                   check=True)
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    dt = load_package().batch.CONTACT_JOINT_DTYPE
    assert int(got["sizeof"]) == dt.itemsize
    for f in fields:
        assert int(got[f]) == dt.fields[f][1], f
    assert dt.names == tuple(n for n, *_ in ld.JOINT_FIELDS)
