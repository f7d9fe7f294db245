"""The per-body flags (DMX_BODY_ALIVE / KINEMATIC / NOGRAVITY / NOGYRO) in every form a dmxBatchStepJoints tick takes, against
the dense float64 reference (tests/lcp_dense.py, whose reading of the flags tests/test_body_flags_reference.py checks on the
CPU), and the refusal of the ticks that find their own contacts (dmx_refuse_flags).

Every solver form wraps its own staging, row build, schedule and force scatter around stage_body / finish_body
(csrc/dmx_island_rows.hpp), so every form gets a scene that mixes all four flags (`flagged`): KINEMATIC on link nb // 2,
NOGRAVITY on link 1, NOGYRO on link nb // 3 with anisotropic inertia and spin everywhere, and one dead slot appended that two
extra joints name -- one from the dead slot to the top link (the dead end is static: body1 is swapped and the normal reversed;
its one row counts among the island's m), one from the dead slot to static ground (dropped).

The harness, tolerances and rules are those of tests/test_gpu_solver_dense.py, unchanged (`check`): 1e-10 float64 QuickStep,
1e-8 float64 dWorldStep, 10 eps32 kappa(A) float32 dWorldStep, the per-body band of tests/quick_band.py for float32 QuickStep
(K eps32 M_v, rows at their bounds included), dead slots bit for bit.  The path a tick took is asserted wherever a
counter says it: lcp_stats()["solves"] (the grid solve) and small_tick_stats() (the single-launch tick or the general path,
with the reason).  Gyro modes: off and implicit everywhere; explicit on the small cases (it overflows on slender spinning
boxes over many ticks, tests/test_gpu_fuzz.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lcp_dense as ld
from __graft_entry__ import load_package
from test_gpu_solver_dense import (PRECS, chain, check, contacts_for_rows, device_tick, lds_boundary, lds_fits, press_chain,
                                   world)

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
EINVAL = -3
AUTO, OFF = B_.SMALL_TICK_AUTO, B_.SMALL_TICK_OFF
GYROS = [ld.GYRO_OFF, ld.GYRO_IMPLICIT]
GYROS3 = [ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT]
SINGLES = [("float64", "quick"), ("float64", "exact"), ("float32", "exact")]     # as test_single_body_on_static_ground


def held(prec, x):
    """x as a batch of this precision holds it"""
    return np.asarray(x, np.float64).astype(prec).astype(np.float64)


def flagged(B, jts, dead_mu=0.0, at=None):
    """-> (Bodies with the four flags placed and one dead slot appended, joints with the two that name it appended).  The
    joint from the dead slot to link `at` (default: the top one) pushes the link sideways, against its velocity (a loaded row)"""
    nb = B.n
    top = nb - 1 if at is None else at
    flags = np.append(B.flags, 0).astype(np.uint8)
    flags[nb // 2 if nb > 1 else 0] |= ld.KINEMATIC
    if nb > 1:
        flags[1] |= ld.NOGRAVITY
    flags[nb // 3] |= ld.NOGYRO
    F = ld.Bodies(np.vstack([B.pos, B.pos[nb - 1] + (0.0, 1.0, 0.0)]), np.vstack([B.quat, [0.6, 0.0, 0.8, 0.0]]),
                  np.vstack([B.lvel, [1.0, 2.0, 3.0]]), np.vstack([B.avel, [0.1, 0.2, 0.3]]), np.append(B.mass, 1.5),
                  np.vstack([B.inertia, [0.3, 0.4, 0.5]]), flags)
    sx = 1.0 if B.lvel[top, 0] >= 0 else -1.0
    extra = np.zeros(2, ld.JOINT_DTYPE)
    extra["pos"] = B.pos[top] + (0.3 * sx, 0.0, 0.0)
    extra["normal"] = (sx, 0.0, 0.0)                    # given as pointing into the dead slot: reversed into the link
    extra["depth"], extra["mu"] = 0.01, (dead_mu, 0.4)
    extra["body1"], extra["body2"] = nb, (top, -1)
    return F, np.concatenate([jts, extra])


def spin(B, rng, scale=0.3):
    B.avel[:] = rng.normal(scale=scale, size=(B.n, 3))
    return B


def run(prec, B, W, jts, stepper, both=False, ticks=1, **kw):
    """check() under the default small-tick mode; with `both` also with the single-launch tick off: the two must agree bit for
    bit (the header's promise) and the counters must name the path.  The kinematic slots' velocities are held bit for bit
    (after a small tick the download is served from the host mirror).  -> check()'s list"""
    res = check(prec, B, W, jts, stepper, ticks=ticks, **kw)
    kin = np.nonzero(((B.flags & ld.KINEMATIC) != 0) & ((B.flags & ld.ALIVE) != 0))[0]
    want = np.column_stack([held(prec, B.lvel), held(prec, B.avel)])[kin]
    for r, st in res:
        assert np.array_equal(r.device[kin, 7:13], want), "a kinematic body's velocity changed"
    if both:
        off = check(prec, B, W, jts, stepper, ticks=ticks, small=OFF, **kw)
        for (r, st), (r2, st2) in zip(res, off):
            assert np.array_equal(r.device, r2.device), "the single-launch tick and the general path differ"
        assert res[-1][1]["tick"]["small"] == ticks and res[-1][1]["tick"]["general"] == 0
        assert off[-1][1]["tick"]["small"] == 0 and off[-1][1]["tick"]["general"] == ticks and off[-1][1]["tick"]["mode"] == ticks
    return res


# ---------------------------------------------------------------------------------------------------------------------
# a. singles: one body on static ground, at the kernel boundaries of test_single_body_on_static_ground
@pytest.mark.parametrize("prec,stepper", SINGLES)
@pytest.mark.parametrize("gyro", GYROS3)
@pytest.mark.parametrize("nc", [1, 5, 8, 9])
def test_single_body_flags(prec, stepper, gyro, nc):
    """the body's flag in turn none, NOGRAVITY, NOGYRO, KINEMATIC (every contact then joins two immovable bodies: the body moves
    with its velocity), and its flagged results differ from the plain one's the way the flag says"""
    out = {}
    for flag in (0, ld.NOGRAVITY, ld.NOGYRO, ld.KINEMATIC):
        rng = np.random.default_rng(100 + nc)
        B, jts = chain(1, nc, np.inf, rng, speed=0.05)
        B.lvel[0] = (0.1, -1.0, 0.0)                 # pressing into the ground: no row near a clamp
        B.avel[0] = (0.7, -0.4, 0.5)
        B.flags[0] |= flag
        (r, st), = run(prec, B, world(prec, gyro=gyro), jts, stepper, both=True)
        out[flag] = r.device
        if flag == ld.KINEMATIC:
            assert np.array_equal(r.device[0, 7:13], np.concatenate([held(prec, B.lvel[0]), held(prec, B.avel[0])]))
            x = held(prec, B.pos[0]) + held(prec, H) * held(prec, B.lvel[0])
            assert np.max(np.abs(r.device[0, 0:3] - x)) <= 2 * np.finfo(prec).eps * np.max(np.abs(x))
    assert not np.array_equal(out[0], out[ld.NOGRAVITY]) and not np.array_equal(out[0], out[ld.KINEMATIC])
    assert np.array_equal(out[0], out[ld.NOGYRO]) == (gyro == ld.GYRO_OFF)


# ---------------------------------------------------------------------------------------------------------------------
# b. QuickStep's forms, float64
def quick_chain(m, seed=None):
    """a pressed chain with friction 0.4, inf and 0 mixed whose island has exactly m rows once `flagged`"""
    rng = np.random.default_rng(m if seed is None else seed)
    mus = contacts_for_rows(m - 1, "mix")
    B, jts = chain(max(2, len(mus) // 3), len(mus), mus, rng, speed=0.02)
    B.lvel[:, 1] -= 1.0 + 0.1 * np.arange(B.n)
    return flagged(spin(B, rng), jts)


def the_island(r, m):
    big = max(r.islands, key=lambda I: I.m)
    assert big.m == m and sum(I.m for I in r.islands) == m, "the flagged scene is one island of m rows"
    return big


@pytest.mark.parametrize("m,gyro", [(m, g) for m in (30, 256, 257, 1536, 1537) for g in GYROS] + [(30, ld.GYRO_EXPLICIT)])
def test_quickstep_forms_f64(m, gyro):
    """the one-wavefront form (<= 256 rows: also the single-launch tick), the register form (<= 1 536) and the one above it"""
    B, jts = quick_chain(m)
    (r, st), = run("float64", B, world("float64", gyro=gyro), jts, "quick", both=m <= 256)
    the_island(r, m)
    if m > 256:
        assert st["tick"]["general"] == 1 and st["tick"]["sor_rows"] == 1


def flagged_press_chain(m, seed):
    """press_chain with the flags, m rows in all (the dead slot's joint makes one, pushing the loaded bottom link sideways
    against a drift of 0.3).  The links are turned at random and spin about the chain's axis: that spin moves no contact point
    along its normal (omega x r is perpendicular to both the axis and r, the normal lies in their plane), so the rows stay as
    loaded as press_chain made them, while omega is off the principal axes and the gyroscopic torque is not zero"""
    rng = np.random.default_rng(seed)
    B, jts = press_chain(m - 1, rng)
    B.quat[:] = [q / np.linalg.norm(q) for q in rng.normal(size=(B.n, 4))]
    B.avel[:, 1] = rng.normal(scale=2.0, size=B.n)
    B.lvel[0, 0] = 0.3
    return flagged(B, jts, at=0)


@pytest.mark.parametrize("gyro", GYROS)
def test_quickstep_above_the_register_form_f64(gyro):
    B, jts = flagged_press_chain(3073, 3073)
    (r, st), = run("float64", B, world("float64", gyro=gyro), jts, "quick")
    the_island(r, 3073)
    assert st["tick"]["general"] == 1 and st["tick"]["bodies"] == 1         # (1 025 live bodies: the first reason that says no)


# c. QuickStep's forms, float32: the row counts of test_quickstep_register_form_f32, its world and its seeds (seed = m)
@pytest.mark.parametrize("gyro", GYROS)
@pytest.mark.parametrize("m", [256, 257, 1025, 3072, 3073])
def test_quickstep_forms_f32(m, gyro):
    """the flagged press_chain in float32, held to the band of tests/quick_band.py"""
    B, jts = flagged_press_chain(m, m)
    (r, st), = run("float32", B, world("float32", gyro=gyro), jts, "quick", both=m <= 256)
    the_island(r, m)


def test_quickstep_lane_per_island_in_a_child_process():
    """DMX_BIG_ISLAND_ROWS=64 (read once per process) sends the 30-row flagged island to the lane-per-island form"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_body_flags as t; "
            "[t.test_quickstep_forms_f64(30, g) for g in t.GYROS3]; print('CHILD-OK')") % (here, os.path.dirname(here))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DMX_BIG_ISLAND_ROWS": "64"})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------------
# d. dWorldStep: the one-workgroup LDS solve and the grid solve
def exact_mus(m):
    return np.append(contacts_for_rows(m - 1, "mix"), 0.0)        # (the last one is the dead slot's joint)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("m,gyro", [(m, g) for m in (63, "last", 300) for g in GYROS] + [(63, ld.GYRO_EXPLICIT)])
def test_exact_forms(prec, m, gyro):
    """63 rows (LDS, also the single-launch tick), the last row count that fits the LDS solve, and ~300 rows: the grid solve"""
    rb = np.dtype(prec).itemsize
    if m == "last":
        m = lds_boundary(rb, exact_mus) - 1
    rng = np.random.default_rng(m)
    mus = exact_mus(m)[:-1]
    B, jts = chain(max(1, len(mus) // 3), len(mus), mus, rng)
    B, jts = flagged(B, jts)
    fits = lds_fits(rb, m, m - 2 * int(np.sum(np.isinf(mus))))
    (r, st), = run(prec, B, world(prec, gyro=gyro), jts, "exact", both=fits)
    big = the_island(r, m)
    assert fits == lds_fits(rb, big.m, big.nbd)
    assert st["solves"] == (0 if fits else 1) and st["fallback"] == 0
    if not fits:
        assert (st["last_m"], st["last_nu"], st["last_nbd"]) == (big.m, big.nu, big.nbd)
        assert st["tick"]["general"] == 1 and st["tick"]["lds_fit"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# e. flags that change between ticks
def flags_change_case():
    rng = np.random.default_rng(61)
    B, jts = chain(80, 160, np.repeat([0.4, 0.0], 80), rng, speed=0.05)       # every link: one contact of 3 rows, one of 1
    spin(B, rng, 0.2)
    B.flags[1] |= ld.NOGRAVITY
    B.flags[26] |= ld.NOGYRO
    return B, jts


FLAGS_OF_BODY_40 = [ld.ALIVE, ld.ALIVE | ld.KINEMATIC, ld.ALIVE, 0, ld.ALIVE, ld.ALIVE]


@pytest.mark.parametrize("prec,stepper", [("float64", "exact"), ("float32", "exact"), ("float64", "quick"), ("float32", "quick")])
def test_flags_change_between_ticks(prec, stepper):
    """six ticks of a resting stack of 80 bodies and 320 rows (dWorldStep: the grid solve, which carries its active set from tick
    to tick); body 40 goes dynamic -> kinematic -> dynamic -> dead -> alive -> alive, every tick equals the reference
    restarted from the device's state with the flags then in force.  The host's mirror of the flags decides which joints
    live (csrc/dmx_joints.cpp), the device's copy how the bodies are staged: both must follow every upload"""
    B, jts = flags_change_case()
    mid = FLAGS_OF_BODY_40

    def between(t, j):
        f = B.flags.copy()
        f[40] = mid[t]
        return j, f

    res = check(prec, B, world(prec, gyro=ld.GYRO_IMPLICIT), jts, stepper, ticks=6, between=between)
    rb, solves, general = np.dtype(prec).itemsize, 0, 0
    for t, (r, st) in enumerate(res):
        # dead: the links into and out of body 40 rest on a static body, two islands of 41 and 39 links
        assert [I.m for I in r.islands] == ([164, 156] if mid[t] == 0 else [320])
        if stepper == "exact":
            grid = any(not lds_fits(rb, I.m, I.nbd) for I in r.islands if I.m)
            assert grid or mid[t] == 0
            assert (st["solves"] > solves) == grid and st["fallback"] == 0
            solves = st["solves"]
        else:
            grid = any(I.m > 256 for I in r.islands)
        general += grid
        assert st["tick"]["general"] == general and st["tick"]["small"] == t + 1 - general


# every float32 QuickStep case of this file with rows: name -> () -> (Bodies, joints, World) of its first tick;
# tests/test_quick_band.py runs the float32 emulation of the reference's sweeps over them (quick_band.MEASURED, population (b));
# the later ticks of flags_change start from the device's state, and are emulated there from the reference's
F32_QUICK_CASES = {"flags_change": lambda: (*flags_change_case(), world("float32", gyro=ld.GYRO_IMPLICIT))}
for _m in (256, 257, 1025, 3072, 3073):
    for _g in GYROS:
        F32_QUICK_CASES[f"flagged_press_chain-{_m}-gyro{_g}"] = lambda m=_m, g=_g: (*flagged_press_chain(m, m), world("float32", gyro=g))


# ---------------------------------------------------------------------------------------------------------------------
# f. bodies without rows
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("gyro", GYROS3)
@pytest.mark.parametrize("ticks", [1, 8])
def test_bodies_without_rows(prec, gyro, ticks):
    """300 bodies, no joints, every flag bit drawn with probability 1/4 (slots 63, 64 and 299 flagged for sure): against the
    reference; the two steppers, and the single-launch tick and the general path (launch_islands_without_rows), bit for bit;
    and bit for bit against a twin without flags on the bodies whose flags are plain -- a flagged neighbour in the same
    wavefront changes nothing"""
    rng = np.random.default_rng(71)
    B, jts = chain(300, 0, 0.0, rng, speed=1.0)
    bits = rng.random((300, 4)) < 0.25
    flags = (np.where(bits[:, 0], 0, ld.ALIVE) | np.where(bits[:, 1], ld.KINEMATIC, 0) | np.where(bits[:, 2], ld.NOGRAVITY, 0)
             | np.where(bits[:, 3], ld.NOGYRO, 0)).astype(np.uint8)
    flags[63], flags[64], flags[299] = ld.ALIVE | ld.KINEMATIC, 0, ld.ALIVE | ld.NOGRAVITY | ld.NOGYRO
    assert all(np.sum((flags & bit) != 0) > 40 for bit in (ld.KINEMATIC, ld.NOGRAVITY, ld.NOGYRO)) and np.sum(flags == ld.ALIVE) > 60
    B.flags[:] = flags
    W = world(prec, gyro=gyro)
    quick = run(prec, B, W, jts, "quick", both=True, ticks=ticks)
    exact = run(prec, B, W, jts, "exact", both=True, ticks=ticks)
    assert np.array_equal(quick[-1][0].device, exact[-1][0].device)
    assert exact[-1][1]["solves"] == 0
    twin = B.copy()
    twin.flags[:] = ld.ALIVE
    plain = flags == ld.ALIVE
    for small in (AUTO, OFF):
        post = device_tick(prec, twin, W, jts, "quick", ticks, small=small)[-1][2]
        assert np.array_equal(post[plain], quick[-1][0].device[plain])
        assert not np.array_equal(post[~plain], quick[-1][0].device[~plain])


# ---------------------------------------------------------------------------------------------------------------------
# the ticks that find their own contacts refuse (dmx_refuse_flags)
def _slab_world():
    """32 boxes in free flight in slots [0, 32) and ghost slots behind them (test_chunk_api_rollback_restores_own_and_ghost_slots)"""
    scene = pkg.scenes.box_grid(8, 4, seed=3, y_range=(5.0, 6.0), spin=True, plane=False).astype("float32")
    L = pkg.shard.SlabLayout(8, 4)
    w = pkg.BatchWorld(L.n_total, dtype="float32")
    w.load_scene(scene)
    g = scene.slice(scene.n - 8, scene.n)
    gpos = g.pos.copy(); gpos[:, 2] += 2.5
    first = int(L.ghost_hi[0])
    w.upload(B_.POS, gpos, first=first)
    w.upload(B_.SIDES, g.sides, first=first)
    w.upload_geom_type(g.gtype, first=first)
    w.set_active_count(scene.n)
    return w, scene.n, first


def _entries(w, n):
    return [("dmxBatchStep", lambda: w.step(H, 1)), ("dmxBatchStepTimed", lambda: w.step_timed(H, 1)),
            ("dmxBatchStepRange", lambda: w.step_range(H, 0, n)), ("dmxBatchChunkTick", lambda: w.chunk_tick(H, True)),
            ("dmxBatchChunkTicks", lambda: w.chunk_ticks(H, 2, True, True)), ("dmxBatchExactTick", lambda: w.exact_tick(H))]


NOT_PLAIN = [0, ld.ALIVE | ld.KINEMATIC, ld.ALIVE | ld.NOGRAVITY, ld.ALIVE | ld.NOGYRO]


@pytest.mark.parametrize("byte", NOT_PLAIN)
def test_ticks_that_do_not_know_flags_say_so(byte, capfd):
    """each of the six entry points, the byte on slot 0 and on the last active slot: DMX_EINVAL, one line on stderr that names
    the call, the count and dmxBatchStepJoints, and the state as it was"""
    w, n, ghost = _slab_world()
    try:
        assert w.chunk_begin() == (False, True)               # (a chunk is open: the chunk ticks have nothing else to object to)
        before = w.download(B_.STATE)
        for slots in ([0], [n - 1], [0, n - 1]):
            f = np.full(n, ld.ALIVE, np.uint8)
            f[slots] = byte
            w.upload_body_flags(f)
            for name, call in _entries(w, n):
                capfd.readouterr()
                with pytest.raises(B_.DmxError) as e:
                    call()
                assert e.value.code == EINVAL
                err = capfd.readouterr().err
                assert err.count("\n") == 1 and f" {name} " in err and "use dmxBatchStepJoints" in err and f" {len(slots)} slot(s)" in err, err
            assert np.array_equal(w.download(B_.STATE), before)
        w.upload_body_flags(np.full(1, ld.ALIVE, np.uint8), first=0)          # one of the two set back: still refused
        with pytest.raises(B_.DmxError):
            w.step(H, 1)
        w.upload_body_flags(np.full(1, ld.ALIVE, np.uint8), first=n - 1)      # both: every entry works again
        capfd.readouterr()
        w.chunk_tick(H, True); w.chunk_ticks(H, 2, True, True)
        assert w.chunk_end() == (False, False)
        w.chunk_commit(3)
        w.step(H, 1); w.step_timed(H, 1); w.step_range(H, 0, n); w.exact_tick(H)
        w.synchronize()
        assert capfd.readouterr().err == ""
        assert not np.array_equal(w.download(B_.STATE)[:n], before[:n])
    finally:
        w.close()


def test_a_flagged_ghost_slot_is_nobodys_business():
    """the only slot that is not plain is a ghost slot: nobody steps it, nobody refuses; and the count follows the active count"""
    w, n, ghost = _slab_world()
    try:
        for byte in NOT_PLAIN:
            w.upload_body_flags(np.full(1, byte, np.uint8), first=ghost)
            assert w.chunk_begin() == (False, True)
            w.chunk_tick(H, True); w.chunk_ticks(H, 2, True, True)
            assert w.chunk_end() == (False, False)
            w.chunk_commit(3)
            w.step(H, 1); w.step_timed(H, 1); w.step_range(H, 0, n); w.exact_tick(H)
        w.synchronize()
        w.set_active_count(w.n)                               # the ghost slots become active ones: now it counts
        with pytest.raises(B_.DmxError) as e:
            w.step(H, 1)
        assert e.value.code == EINVAL
        w.set_active_count(n)
        w.step(H, 1)
        w.synchronize()
    finally:
        w.close()


@pytest.mark.parametrize("dtype", PRECS)
def test_after_a_refusal_the_batch_runs_as_if_nothing_happened(dtype):
    """flags set, a refused tick, flags set back: 40 ticks of 64 boxes falling onto the plane and each other equal a twin that
    never had flags, bit for bit, and so do the collision statistics"""
    scene = pkg.scenes.box_grid(8, 8, seed=1, y_range=(0.6, 1.5), spin=True, box_mass=True).astype(dtype)
    out = []
    for touched in (False, True):
        w = pkg.BatchWorld(scene.n, dtype=dtype)
        try:
            w.load_scene(scene)
            w.set_body_collisions(True)
            if touched:
                f = np.full(scene.n, ld.ALIVE, np.uint8)
                f[5], f[63] = ld.ALIVE | ld.KINEMATIC, 0
                w.upload_body_flags(f)
                with pytest.raises(B_.DmxError):
                    w.step(H, 40)
                w.upload_body_flags(np.full(scene.n, ld.ALIVE, np.uint8))
            w.step(H, 40)
            w.synchronize()
            out.append((w.download(B_.STATE), w.collision_stats(), w.last_contact_count()))
        finally:
            w.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][2] == out[1][2]
    assert out[0][2] > 0 and out[0][1]["fast_ticks"] + out[0][1]["careful_ticks"] > 0
