"""The single-launch tick of small worlds (csrc/dmx_small.hip; dmxBatchSetSmallTick / dmxBatchSmallTickStats).

A dmxBatchStepJoints tick of a world of a few hundred bodies at most runs as ONE kernel launch: tables read from host-mapped
staging, the new state written to the slab and to a host-mapped mirror that dmxBatchDownload serves state fields from.  The
kernel calls the device functions the general path's kernels wrap, so the two paths must give the same bits.

  1. the path is taken and says so (DMX_SMALL_TICK_REPORT);
  2. same answer as the general path (DMX_SMALL_TICK=0): np.array_equal for QuickStep AND for dWorldStep -- the LDS solve's
     device function is shared unchanged and runs in the same 256-thread workgroup shape, so no reduction order differs;
  3. same answer as the checkers: the oracle through the ODE API (QuickStep bit for bit, dWorldStep within 1e-5, what
     tests/test_ode_compat.py asserts for the general path), and tests/lcp_dense.py on synthetic joints with the tolerances
     written at the top of tests/test_gpu_solver_dense.py (f64 QuickStep 1e-10, f64 dWorldStep 1e-8, f32 dWorldStep 10 eps32
     kappa, f32 QuickStep the per-body band of tests/quick_band.py, rows at their bounds included);
  4. the mirror is never stale; 5. eligibility falls back, never fails; 6. two worlds in one process.

The DMX_* knobs are read once per process, so runs with DMX_SMALL_TICK=0 / DMX_ROW_ORDER go through the C harness
(tests/harness/ode_tick_harness.c), a process of its own."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lcp_dense as ld
import quick_band as qb
from __graft_entry__ import load_package
from test_ode_compat import _build_harness, _scene_text, _oracle_poses, _rel

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

DT = 1.0 / 120.0
EPS32 = float(np.finfo(np.float32).eps)
_TMP = tempfile.mkdtemp(prefix="small_tick_")


@functools.lru_cache(maxsize=None)
def _exe(single):
    return _build_harness(_TMP, single)


def _run(single, text, stepper, env=None):
    """-> (poses (n, 16), the library's report counters summed over the world's batches) of one harness process"""
    p = subprocess.run([_exe(single)], input=text, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "HARNESS_STEPPER": stepper, "DMX_SMALL_TICK_REPORT": "1", **(env or {})})
    assert p.returncode == 0, p.stderr[-2000:]
    poses = np.array([[float(v) for v in line.split()] for line in p.stdout.strip().splitlines()])
    lines = re.findall(r"small tick: (.*)", p.stderr)
    assert lines, "no `small tick:` report line on stderr:\n" + p.stderr[-1000:]
    rep = dict.fromkeys(B_.SMALL_TICK_STATS, 0)
    for line in lines:                  # one line per batch destroyed: a world that outgrows its batch makes a larger one
        for kv in line.split():
            k, v = kv.split("=")
            rep[k] += int(v)
    return poses, rep


STEPS = 300


@functools.lru_cache(maxsize=None)
def _pen(n, single, stepper, small):
    """the reference's map with n spawned bodies, STEPS ticks, on the single-launch path or with DMX_SMALL_TICK=0"""
    statics, bodies = pkg.scenes.reference_map(), pkg.scenes.reference_spawn(n, seed=7)
    return _run(single, _scene_text(DT, STEPS, False, statics, bodies), stepper, env={"DMX_SMALL_TICK": "1" if small else "0"})


PEN = [pytest.param(n, single, stepper, id=f"{n}-{'f32' if single else 'f64'}-{stepper}")
       for n in (3, 24, 48) for single in (False, True) for stepper in ("quick", "exact")]


# --------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n,single,stepper", PEN)
def test_path_is_taken_and_says_so(n, single, stepper):
    _, rep = _pen(n, single, stepper, True)
    assert rep["general"] == 0 and rep["small"] == STEPS, rep
    assert all(rep[k] == 0 for k in B_.SMALL_TICK_STATS[2:]), rep
    _, off = _pen(n, single, stepper, False)
    assert off["small"] == 0 and off["general"] == STEPS and off["mode"] == STEPS, off


# --------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n,single,stepper", PEN)
def test_same_answer_as_the_general_path(n, single, stepper):
    got, _ = _pen(n, single, stepper, True)
    ref, _ = _pen(n, single, stepper, False)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, ref), np.abs(got - ref).max()


# --------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n,single,stepper", PEN)
def test_same_answer_as_the_oracle(n, single, stepper):
    dtype = "float32" if single else "float64"
    statics, bodies = pkg.scenes.reference_map(), pkg.scenes.reference_spawn(n, seed=7)
    got, _ = _pen(n, single, stepper, True)
    ref, _ = _oracle_poses(dtype, DT, STEPS, False, statics, bodies, exact=stepper == "exact")
    if stepper == "quick":
        assert np.array_equal(got.astype(ref.dtype), ref), np.abs(got - ref).max()
    else:
        err = _rel(got.astype(ref.dtype), ref)
        print(f"dWorldStep {n} bodies {dtype}: rel err vs the oracle's exact stepper {err:.3e}")
        assert err <= 1e-5


# ---- synthetic joints against the dense reference
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _chain(nb, n_contacts, mu, rng, mode=ld.CONTACT_BOUNCE, speed=0.05, press=True):
    """nb bodies in a chain along y (slot k rests on k - 1, slot 0 on static ground), n_contacts contacts spread round-robin
    over the links, `mu` a number or a per-contact array; every body moving into the one below, so no row sits at a clamp"""
    pos = np.column_stack([rng.uniform(-0.05, 0.05, nb), 0.5 + np.arange(nb), rng.uniform(-0.05, 0.05, nb)])
    quat = np.array([_unit(rng.normal(size=4)) for _ in range(nb)])
    lv = rng.normal(scale=speed, size=(nb, 3))
    if press:
        lv[:, 1] = -(1.0 + 0.1 * np.arange(nb))
    B = ld.Bodies(pos, quat, lv, rng.normal(scale=speed, size=(nb, 3)), rng.uniform(0.5, 2.0, nb), rng.uniform(0.2, 1.0, (nb, 3)))
    links = [(0, -1)] + [(k, k - 1) for k in range(1, nb)]
    mus = np.broadcast_to(np.asarray(mu, np.float64), (n_contacts,))
    out = []
    for c in range(n_contacts):
        b1, b2 = links[c % len(links)]
        axis = B.pos[b1] - B.pos[b2] if b2 >= 0 else np.array([0.0, 1.0, 0.0])
        nrm = _unit(_unit(axis) + 0.4 * _unit(rng.normal(size=3)))
        p = B.pos[b1] + 0.6 * rng.uniform(0.2, 1.0) * _unit(rng.normal(size=3))
        out.append((p, nrm, rng.uniform(0, 0.05), b1, b2, mode, mus[c], 0.2, 0.1, 0.0, 0.0))
    return B, np.array(out, ld.JOINT_DTYPE)


def _join(parts, dx=10.0):
    """several (Bodies, joints) side by side in one world: separate islands that share the static ground"""
    Bs, js, off = [], [], 0
    for k, (B, j) in enumerate(parts):
        B = B.copy(); j = j.copy()
        B.pos[:, 0] += dx * k; j["pos"][:, 0] += dx * k
        j["body1"] += off; j["body2"] = np.where(j["body2"] >= 0, j["body2"] + off, -1)
        Bs.append(B); js.append(j); off += B.n
    B = ld.Bodies(*[np.vstack([getattr(b, f) for b in Bs]) for f in ("pos", "quat", "lvel", "avel")],
                  np.concatenate([b.mass for b in Bs]), np.vstack([b.inertia for b in Bs]), np.concatenate([b.flags for b in Bs]))
    return B, np.concatenate(js)


def _new_world(prec, B, W, stepper):
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
    w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
    w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
    w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
    w.upload_body_flags(B.flags)
    return w


def _as_precision(prec, W, jts):
    if np.dtype(prec).itemsize == 8:
        return W, jts
    r = lambda x: float(np.float32(x))
    W2 = ld.World(h=r(W.h), gravity=np.asarray(W.gravity, np.float32).astype(np.float64), erp=r(W.erp), cfm=r(W.cfm),
                  iters=W.iters, sor_w=r(W.sor_w), gyro=W.gyro)
    j2 = jts.copy()
    for f in ("pos", "normal", "depth", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"):
        j2[f] = np.asarray(jts[f], np.float32).astype(np.float64)
    return W2, j2


DEVICE_WORST = {"contact": 0.0}          # the largest device deviation of this process, in eps32 M_v (printed by _dense)


def _dense(prec, B, jts, stepper, W=None):
    """one step_joints tick on a fresh batch against tests/lcp_dense.py run from the device's own pre-tick state.
    -> (reference Result, post-tick state (n, 13), small_tick_stats, lcp_stats)"""
    W = W or ld.World(cfm=1e-5)
    w = _new_world(prec, B, W, stepper)
    try:
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        pre = w.download(B_.STATE).astype(np.float64)
        w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE))
        post = w.download(B_.STATE).astype(np.float64)          # (a small tick: served from the mirror, after the wait)
        stats, lcp = w.small_tick_stats(), w.lcp_stats()
        contacts = w.last_contact_count()
    finally:
        w.close()
    Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, B.flags)
    Wr, jr = _as_precision(prec, W, jts)
    r = ld.step(Bp, Wr, jr, stepper)
    f32 = np.dtype(prec).itemsize == 4
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    if f32 and stepper == "quick":
        worst = qb.assert_in_band(r, Wr, post, qb.K["contact"], live)
        DEVICE_WORST["contact"] = max(DEVICE_WORST["contact"], worst)
        print(f"f32 QuickStep, single-launch tick: {worst:.2f} eps32 M_v (K = {qb.K['contact']}; largest so far "
              f"{DEVICE_WORST['contact']:.2f})")
    else:
        t = (1e-10 if stepper == "quick" else 1e-8) if not f32 else 10 * EPS32 * max([I.kappa() for I in r.islands] + [1.0])
        scale = ld.velocity_scale(r.bodies, Wr, live)
        err = ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13], live)
        assert err <= t * scale, f"velocity error {err:.3e} > {t:.1e} x {scale:.3e}"
        eps = 4 * (EPS32 if f32 else 2.2e-16)
        xerr = np.max(np.abs(post[live, 0:3] - r.bodies.pos[live]))
        assert xerr <= t * scale * Wr.h + eps * max(1.0, np.max(np.abs(r.bodies.pos[live]))), f"position error {xerr:.3e}"
        qerr = np.max(np.abs(post[live, 3:7] - r.bodies.quat[live]))
        assert qerr <= t * scale * Wr.h + eps, f"quaternion error {qerr:.3e}"
    dead = np.nonzero(~(Bp.flags & ld.ALIVE).astype(bool))[0]
    if len(dead):
        assert np.array_equal(post[dead], pre[dead]), "a dead slot changed"
    assert contacts == sum(len(set(I.row_joint.tolist())) for I in r.islands if I.m), "StepDiag's contact count"
    return r, post, stats, lcp


def _on_small_path(stats):
    assert stats["small"] == 1 and stats["general"] == 0 and sum(stats[k] for k in B_.SMALL_TICK_STATS[2:]) == 0, stats


COMBOS = [("float64", "quick"), ("float64", "exact"), ("float32", "exact"), ("float32", "quick")]


def _singles_case(nc):
    rng = np.random.default_rng(100 + nc)
    return _join([_chain(1, nc, np.inf, rng), _chain(1, 0, 0.0, rng)])


@pytest.mark.parametrize("prec,stepper", COMBOS)
@pytest.mark.parametrize("nc", range(1, 9))
def test_dense_single_body_islands(prec, stepper, nc):
    """one body with 1..8 contacts on static ground (QuickStep: the lane forms in the kernel's tail) beside a free body.  (nc = 1
    under QuickStep has converged long before the last sweep: it cannot show a dropped sweep, the other seven can.)"""
    B, jts = _singles_case(nc)
    r, post, stats, _ = _dense(prec, B, jts, stepper)
    _on_small_path(stats)
    assert sorted(I.m for I in r.islands) == [0, 3 * nc]


def _press_chain_case():
    rng = np.random.default_rng(7)
    nb = 8
    pos = np.column_stack([np.zeros(nb), 0.5 + np.arange(nb), np.zeros(nb)])
    lv = np.zeros((nb, 3)); lv[:, 1] = -(1.0 + 0.1 * np.arange(nb))
    B = ld.Bodies(pos, np.tile([1.0, 0, 0, 0], (nb, 1)), lv, np.zeros((nb, 3)), rng.uniform(0.8, 1.2, nb), rng.uniform(0.3, 0.5, (nb, 3)))
    out = []
    for c in range(3 * nb):
        k = c // 3
        a = 2 * np.pi * (c % 3) / 3 + 0.3 * k
        d = np.array([np.cos(a), 0.0, np.sin(a)])
        out.append((np.array([0.0, float(k), 0.0]) + 0.3 * d, np.array([0.0, np.cos(0.6), 0.0]) + d * np.sin(0.6), 0.01, k, k - 1 if k else -1,
                    0, 0.0, 0, 0, 0, 0))
    return B, np.array(out, ld.JOINT_DTYPE)


@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_dense_press_chain_f32(stepper):
    """float32, both steppers, on a multi-body island whose rows all stay loaded"""
    B, jts = _press_chain_case()
    _, _, stats, _ = _dense("float32", B, jts, stepper)
    _on_small_path(stats)


def _kinematic_case(prec):
    rng = np.random.default_rng(21)
    B1, j1 = _chain(3, 9, 0.4, rng)
    n = 4
    flags = np.full(n, ld.ALIVE, np.uint8); flags[0] |= ld.KINEMATIC
    B = ld.Bodies(np.vstack([[[0, -0.5, 0]], B1.pos]), np.vstack([[[1, 0, 0, 0]], B1.quat]), np.vstack([[[0.1, 0.2, 0]], B1.lvel]),
                  np.vstack([[[0, 0.3, 0]], B1.avel]), np.concatenate([[5.0], B1.mass]), np.vstack([[[1, 1, 1]], B1.inertia]), flags)
    jj = j1.copy()
    jj["body1"] += 1; jj["body2"] = np.where(j1["body2"] >= 0, j1["body2"] + 1, 0)
    for f in ("pos", "quat", "lvel", "avel", "mass", "inertia"):
        setattr(B, f, getattr(B, f).astype(prec).astype(np.float64))
    return B, jj


@pytest.mark.parametrize("prec,stepper", COMBOS)
def test_dense_kinematic_body_under_a_stack(prec, stepper):
    B, jj = _kinematic_case(prec)
    r, post, stats, _ = _dense(prec, B, jj, stepper)
    _on_small_path(stats)
    assert np.array_equal(post[0, 7:13], np.concatenate([B.lvel[0], B.avel[0]]))          # the kinematic body keeps its velocity


def _surfaces_case():
    rng = np.random.default_rng(11)
    parts = []
    for k in range(2):
        B, j = _chain(4, 12, np.array([0.0, 0.5, np.inf] * 4), rng, speed=0.3)
        j["mode"] = np.array([ld.CONTACT_BOUNCE, 0, ld.CONTACT_SOFT_ERP | ld.CONTACT_BOUNCE, ld.CONTACT_SOFT_CFM] * 3)
        j["bounce"], j["bounce_vel"], j["soft_erp"], j["soft_cfm"] = 0.7, 0.05, 0.8, 1e-3
        parts.append((B, j))
    return _join(parts)


@pytest.mark.parametrize("prec,stepper", COMBOS)
def test_dense_per_contact_surfaces_in_two_islands_sharing_a_static(prec, stepper):
    """per-contact mu 0 / finite / inf, bounce on and off, soft ERP and soft CFM, in two islands that both rest on the static
    ground"""
    r, _, stats, _ = _dense(prec, *_surfaces_case(), stepper)
    _on_small_path(stats)
    assert sorted(I.m for I in r.islands) == [28, 28]


# every float32 QuickStep case _dense runs: name -> () -> (Bodies, joints, World); tests/test_quick_band.py runs the float32
# emulation of the reference's sweeps over them (population (b) of quick_band.MEASURED)
F32_QUICK_CASES = {"press_chain": lambda: (*_press_chain_case(), ld.World(cfm=1e-5)),
                   "kinematic": lambda: (*_kinematic_case("float32"), ld.World(cfm=1e-5)),
                   "surfaces": lambda: (*_surfaces_case(), ld.World(cfm=1e-5))}
for _nc in range(1, 9):
    F32_QUICK_CASES[f"singles-{_nc}"] = lambda nc=_nc: (*_singles_case(nc), ld.World(cfm=1e-5))


def _lds_fits(real_bytes, m, nbd, lim=150 * 1024):
    """csrc/dmx_lcp.hip lcp_lds_fits"""
    if m + 1 > (288 if real_bytes == 4 else 192):
        return False
    nu = m - nbd
    reals = (m + 1) * (m + 2) // 2 + (nbd + 1) * (nbd + 2) // 2 + 4 * nbd + nu + max(nu, 2 * nbd) + 8
    return ((reals * real_bytes + 15) // 16) * 16 + (3 * m + 3 * nbd + 16) * 4 <= lim


@pytest.mark.parametrize("prec", ["float64", "float32"])
@pytest.mark.parametrize("where", ["last", "over"])
def test_dense_exact_island_at_the_lds_limit(prec, where):
    """frictionless contacts, one row each (every row bounded): the largest island lcp_lds_fits accepts runs on the single-launch
    path, one more row sends the whole tick to the general path (the grid solve) and the LDS-fit reason is counted"""
    rb = np.dtype(prec).itemsize
    m = 1
    while _lds_fits(rb, m + 1, m + 1):
        m += 1
    assert _lds_fits(rb, m, m) and not _lds_fits(rb, m + 1, m + 1)
    m = m if where == "last" else m + 1
    B, jts = _chain(max(1, m // 3), m, 0.0, np.random.default_rng(m))
    r, _, stats, lcp = _dense(prec, B, jts, "exact")
    assert max(I.m for I in r.islands) == m
    if where == "last":
        _on_small_path(stats)
        assert lcp["solves"] == 0
    else:
        assert stats["small"] == 0 and stats["general"] == 1 and stats["lds_fit"] == 1, stats
        assert lcp["solves"] == 1


# --------------------------------------------------------------------------------------------------------------------- 4
def _ground_joints(pos, mu=np.inf):
    """one contact per body with the static ground, under the body"""
    n = len(pos)
    j = ld.joints(n, normal=(0.0, 1.0, 0.0), depth=0.01, mode=ld.CONTACT_BOUNCE, mu=mu, bounce=0.2, bounce_vel=0.1, body2=-1)
    j["body1"] = np.arange(n)
    j["pos"] = np.asarray(pos, np.float64) - (0.0, 0.3, 0.0)
    return j.astype(B_.CONTACT_JOINT_DTYPE)


@pytest.mark.parametrize("prec", ["float64", "float32"])
@pytest.mark.parametrize("stepper", [B_.STEPPER_QUICK, B_.STEPPER_EXACT])
def test_mirror_is_never_stale(prec, stepper):
    """one batch, small ticks interleaved with every other kind of writer of body state; after each, what state() returns (from
    the mirror when it is valid) equals the state of a twin batch whose mode is OFF -- every download of the twin packs the
    slab on the device -- fed the same calls"""
    scene = pkg.scenes.box_grid(4, 4, seed=3, y_range=(0.6, 1.5), spin=True, box_mass=True).astype(prec)
    h = np.dtype(prec).type(1.0 / 60.0)
    a, t = B_.BatchWorld(scene.n, prec), B_.BatchWorld(scene.n, prec)
    try:
        for w in (a, t):
            w.load_scene(scene)
            w.set_stepper(stepper)
        t.set_small_tick(B_.SMALL_TICK_OFF)
        jts = _ground_joints(scene.pos)

        def same(what):
            sa, st = a.state(), t.state()
            for name, x, y in zip(("pos", "quat", "lvel", "avel"), sa, st):
                assert np.array_equal(x, y), (what, name, np.abs(x - y).max())
            assert np.array_equal(a.download(B_.STATE), t.download(B_.STATE)), what
            assert np.array_equal(a.download(B_.STATE, 5, 7), t.download(B_.STATE)[5:12]), what          # a sub-range of the mirror
            assert a.last_contact_count() == t.last_contact_count(), what
            return sa

        def both(f):
            f(a); f(t)

        both(lambda w: w.step_joints(h, jts)); same("small tick")
        assert a.small_tick_stats()["small"] == 1
        new_pos = scene.pos + np.array([0.25, 0.5, -0.25], scene.pos.dtype)
        both(lambda w: w.upload(B_.POS, new_pos))
        assert np.array_equal(same("upload")[0], new_pos)
        both(lambda w: w.step_joints(h, jts)); same("small tick after an upload")
        a.set_small_tick(B_.SMALL_TICK_OFF)
        both(lambda w: w.step_joints(h, jts)); same("tick forced general")
        a.set_small_tick(B_.SMALL_TICK_AUTO)
        both(lambda w: w.step_joints(h, jts)); same("small tick after a general one")
        both(lambda w: w.step(h, 3)); same("the batch's own collide + step")
        both(lambda w: w.step_joints(h, jts)); same("small tick after step()")
        both(lambda w: w.upload(B_.LVEL, np.ones((4, 3), scene.pos.dtype), first=3)); same("partial upload of one field")
        flags = np.full(scene.n, B_.BODY_ALIVE, np.uint8); flags[2] = 0; flags[9] |= B_.BODY_KINEMATIC
        both(lambda w: w.upload_body_flags(flags))
        both(lambda w: w.step_joints(h, jts)); same("small tick with a dead and a kinematic slot")
        both(lambda w: w.step_joints(h, jts[:0])); same("small tick without joints")
        sa = a.small_tick_stats()
        assert sa["small"] == 6 and sa["mode"] == 1, sa
        assert t.small_tick_stats()["small"] == 0
    finally:
        a.close(); t.close()


# --------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("single", [False, True])
def test_odes_row_order_takes_the_general_path(single):
    """DMX_ROW_ORDER=ode:3: the shuffled sweeps are sequential over a host-built table -- never the single-launch path; the
    answer is the oracle's ORC_ORDER_ODE mode bit for bit, as before"""
    dtype = "float32" if single else "float64"
    statics, bodies = pkg.scenes.reference_map(), pkg.scenes.reference_spawn(24, seed=7)
    steps = 200
    got, rep = _run(single, _scene_text(DT, steps, False, statics, bodies), "quick", env={"DMX_ROW_ORDER": "ode:3"})
    assert rep["small"] == 0 and rep["general"] == steps and rep["row_order"] == steps, rep
    ref, _ = _oracle_poses(dtype, DT, steps, False, statics, bodies, ode_order_seed=3)
    assert np.array_equal(got.astype(ref.dtype), ref), np.abs(got - ref).max()


@pytest.mark.parametrize("prec", ["float64", "float32"])
def test_more_bodies_than_the_cap_take_the_general_path(prec):
    n = 600                                     # the cap is the reference's MAX_BODIES = 512
    rng = np.random.default_rng(1)
    pos = rng.uniform(-50, 50, (n, 3))
    a, t = B_.BatchWorld(n, prec), B_.BatchWorld(n, prec)
    try:
        t.set_small_tick(B_.SMALL_TICK_OFF)
        for w in (a, t):
            w.upload(B_.POS, pos)
            for _ in range(3):
                w.step_joints(1.0 / 60.0, _ground_joints(pos[:40]))
        sa = a.small_tick_stats()
        assert sa["small"] == 0 and sa["general"] == 3 and sa["bodies"] == 3, sa
        assert np.array_equal(a.download(B_.STATE), t.download(B_.STATE))
    finally:
        a.close(); t.close()


@pytest.mark.parametrize("single", [False, True])
def test_world_that_grows_across_the_cap(single):
    """505 bodies up front, one more every 2 ticks, poses read every tick: ticks 0..15 hold at most 512 bodies (single-launch
    path), from tick 16 on the world has 513 and more (general path); the poses equal the DMX_SMALL_TICK=0 run throughout"""
    up_front, every, steps, n = 505, 2, 40, 525
    bodies = pkg.scenes.reference_spawn(n, seed=5, y_range=(1.2, 400.0))        # sparse: nothing piles up in 40 ticks
    text = _scene_text(DT, steps, True, [], bodies)
    env = {"HARNESS_SPAWN": f"{up_front} {every}", "HARNESS_READBACK": "1"}
    got, rep = _run(single, text, "quick", env={**env, "DMX_SMALL_TICK": "1"})
    ref, off = _run(single, text, "quick", env={**env, "DMX_SMALL_TICK": "0"})
    crossed = (512 - up_front + 1) * every                    # the first tick with 513 bodies
    assert rep["small"] == crossed and rep["general"] == steps - crossed and rep["bodies"] == steps - crossed, rep
    assert off["small"] == 0 and off["general"] == steps
    assert np.all(np.isfinite(got)) and np.array_equal(got, ref), np.abs(got - ref).max()


# --------------------------------------------------------------------------------------------------------------------- 6
def test_two_worlds_in_one_process_ticking_alternately():
    """each batch has its own staging, mirror and diagnostics slots: two worlds ticked alternately end where each ends alone"""
    rng = np.random.default_rng(3)
    cases = [("float64", "quick", _join([_chain(3, 9, 0.5, rng), _chain(1, 4, np.inf, rng)])),
             ("float32", "exact", _join([_chain(2, 6, np.inf, rng), _chain(1, 0, 0.0, rng), _chain(4, 10, 0.3, rng)]))]
    W = ld.World(cfm=1e-5)
    ticks = 6

    def make(k):
        prec, stepper, (B, jts) = cases[k]
        return _new_world(prec, B, W, stepper), jts.astype(B_.CONTACT_JOINT_DTYPE)

    alone = []
    for k in range(2):
        w, j = make(k)
        try:
            hist = []
            for _ in range(ticks):
                w.step_joints(W.h, j)
                hist.append((w.download(B_.STATE), w.last_contact_count()))
            alone.append(hist)
        finally:
            w.close()
    (w0, j0), (w1, j1) = make(0), make(1)
    try:
        for s in range(ticks):
            w0.step_joints(W.h, j0)
            w1.step_joints(W.h, j1)                 # (both kernels in flight before either mirror is read)
            for k, w in ((0, w0), (1, w1)):
                state, contacts = alone[k][s]
                assert np.array_equal(w.download(B_.STATE), state), (k, s)
                assert w.last_contact_count() == contacts
        for w in (w0, w1):
            st = w.small_tick_stats()
            assert st["small"] == ticks and st["general"] == 0, st
    finally:
        w0.close(); w1.close()
