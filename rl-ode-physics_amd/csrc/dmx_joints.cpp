// dmx_joints.cpp -- dmxBatchStepJoints: one tick driven by an explicit list of contact joints (the form the
// reference's near callback produces, /root/reference/src/main.c:683-692, followed by dWorldStep, main.c:213).
//
// Host work is bookkeeping only: group bodies into dynamics islands (union-find over joints that connect two
// dynamic bodies; static geometry does not link islands), order islands / bodies / joints canonically
// (islands by lowest slot, bodies ascending, joints in creation order), copy the arrays to the device and
// launch solve_islands.  All arithmetic of the step runs on the GPU.
#include <string.h>
#include <memory>
#include <numeric>

#include "dmx_batch_priv.hpp"
#include "dmx_lcp.hpp"
#include "dmx_small.hpp"

namespace {


// multi-body islands with at least this many rows get a workgroup and a level schedule (DMX_BIG_ISLAND_ROWS overrides, for
// tests).  One lane walking an island pays a dependent L2 round trip per row and sweep, so every island with rows is better
// off with a wavefront: 500-body reference scene 5.2 / 3.3 / 2.4 / 1.7 / 1.3 / 1.1 / 0.8 ms per tick at 384 / 128 / 64 / 32 / 16 /
// 8 / 4 rows (profiles/r01_big_island_threshold.txt), 0.90 -> 0.67 from 4 to 1 with the one-body islands on solve_singles
// (profiles/r02_island_threshold.txt).
int big_island_rows()
{
    static const int v = [] { const char *e = getenv("DMX_BIG_ISLAND_ROWS"); return e ? atoi(e) : 1; }();
    return v;
}

// union-find over body slots on a parent array that persists between ticks (identity outside a tick: only the entries
// a tick touched are put back, so a tick costs O(bodies involved), not O(bodies of the batch))
struct UnionFind {
    std::vector<int> &p;
    explicit UnionFind(std::vector<int> &parent) : p(parent) {}
    int find(int x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }
    void unite(int a, int b) { a = find(a); b = find(b); if (a != b) { if (a < b) p[b] = a; else p[a] = b; } }
};

int ensure_pinned(void **p, size_t *have, size_t bytes)
{
    if (bytes <= *have) return DMX_OK;
    if (*p) HIP_TRY(hipHostFree(*p));
    *p = nullptr; *have = 0;
    size_t want = bytes + bytes / 2 + 256;
    HIP_TRY(hipHostMalloc(p, want));
    *have = want;
    return DMX_OK;
}

// the same for host-mapped memory (hipHostMallocMapped) and its device address
int ensure_mapped(void **p, void **dev, size_t *have, size_t bytes)
{
    if (bytes <= *have) return DMX_OK;
    if (*p) HIP_TRY(hipHostFree(*p));
    *p = nullptr; *dev = nullptr; *have = 0;
    size_t want = bytes + bytes / 2 + 4096;
    HIP_TRY(hipHostMalloc(p, want, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(dev, *p, 0));
    *have = want;
    return DMX_OK;
}

template <class T> int step_joints_t(dmxBatch *b, double h, int64_t nj_in, const dmxContactJoint *joints,
                                     const uint8_t *include, const DevGeometry *geo, const dmxContactSurface *surfaces)
{
    const int n = (int)b->n;
    // feedback (dmxBatchSetFeedback): for dmxBatchStepJoints' own ticks only -- the ticks that find their contacts themselves come
    // here with a subset or with device geometry, and produce none.  Off, nothing below stages, launches or stores anything new.
    const bool fb = b->fb_on && !include && !geo;
    const bool fb_was_valid = b->fb_valid;  // (a tick refused before it touches anything leaves the last tick's feedback served)
    b->fb_valid = false;                    // (set again where the tick has been enqueued whole)
    bool exact = b->stepper_exact;          // dWorldStep: islands solved exactly (decided per tick: see the row limit below)
    // per-slot scratch that persists between ticks: parent = identity, island = -1, last = -1 outside a tick
    if ((int)b->sc_parent.size() != n) {
        b->sc_parent.resize((size_t)n); std::iota(b->sc_parent.begin(), b->sc_parent.end(), 0);
        b->sc_island.assign((size_t)n, -1);
        b->sc_last.assign((size_t)n, -1);
    }
    // ---- canonical joints: body1 is a live dynamic slot, normal points into it -----------------------
    std::unique_ptr<DmxPhase> ph(new DmxPhase(b, 4));
    // (all per-tick work arrays below are members of the batch, reused from tick to tick: tens of MB of fresh
    // allocations per tick would be handed back to the OS and page-faulted in again every time)
    typedef DmxCanonicalJoint CJ;
    std::vector<CJ> &cj = b->sc_cj;
    cj.clear();
    cj.reserve((size_t)nj_in);
    // `include` (optional) restricts the tick to a subset of bodies: the rest is stepped by the fused kernels
    auto live = [&](int s) { return s >= 0 && s < n && (b->h_bflags[(size_t)s] & BF_ALIVE) && (!include || include[s]); };
    // the active articulation joints first, as units of at most three rows (a ball: one unit; a hinge: its ball unit, the two
    // angular rows and, when its limot is present, the limit / motor row; a slider: the angular lock, the two linear rows and, when
    // present, its limot row; a fixed joint: a ball unit and the lock), in the order of the set: the stable sort by island below
    // keeps them ahead of the island's contacts
    if (!b->art.empty() && (include || geo)) {          // (every caller that steps a subset is refused before it gets here)
        fprintf(stderr, "libode_mi355: a tick of a subset of the bodies does not honour articulation joints (dmxBatchSetJoints)\n");
        return DMX_EINVAL;
    }
    { const int rc_ad = dmx_ad_merge(b); if (rc_ad != DMX_OK) return rc_ad; }      // (the islands below are judged by the bytes the last tick left)
    int n_limots = 0;
    // angular motors (dmxBatchSetAMotors): one unit of one row per axis whose limot is present; n_amotor_rows > 0 is what sends
    // amotor_prepare in front of the tick.  An active AMotor between two bodies links them whether it has a row or not: am_links
    std::vector<std::pair<int, int>> &am_links = b->sc_am_links;
    am_links.clear();
    int n_amotor_rows = 0;
    if (!b->art.empty()) {
        for (size_t a = 0; a < b->art.size(); a++) {
            const dmxJoint &j = b->art[a];
            int b1 = j.body1, b2 = j.body2;
            if ((b1 < 0 && b2 < 0) || b1 == b2) continue;
            if ((b1 >= 0 && !live(b1)) || (b2 >= 0 && !live(b2))) continue;
            const bool rev = b1 < 0;
            if (rev) { b1 = b2; b2 = -1; }
            DmxCanonicalJoint u; u.b1 = b1; u.b2 = b2; u.j = nullptr; u.rev = rev; u.unit = UNIT_BALL; u.art = (int)a;
            if (j.kind == DMX_JOINT_AMOTOR) {
                if (b2 >= 0) am_links.push_back({ b1, b2 });
                if (b->amotor.empty()) continue;
                for (int i = 0; i < 3; i++)
                    if (dmx_amotor_present(b->amotor[a], i)) { u.unit = UNIT_AMOTOR; u.axis = i; cj.push_back(u); n_limots++; n_amotor_rows++; }
                continue;
            }
            const bool limot = !b->limot.empty() && dmx_limot_present(b->limot[a]);
            if (j.kind == DMX_JOINT_SLIDER) {
                // lock (3), linear (2), limot (1 if present): the limot's entry reads its anchors from the linear unit before it
                u.unit = UNIT_LOCK; cj.push_back(u);
                u.unit = UNIT_SLIDER2; cj.push_back(u);
                if (limot) { u.unit = UNIT_SLIMOT; cj.push_back(u); n_limots++; }
                continue;
            }
            cj.push_back(u);
            if (j.kind == DMX_JOINT_HINGE) {
                u.unit = UNIT_HINGE2; cj.push_back(u);
                if (limot) { u.unit = UNIT_LIMOT; cj.push_back(u); n_limots++; }
            } else if (j.kind == DMX_JOINT_FIXED) {
                u.unit = UNIT_LOCK; cj.push_back(u);
            }
        }
    }
    int n_units = (int)cj.size();
    // rows of an entry, and how many of them can clamp (a limot unit's one row is counted as able to, whatever its state will be)
    auto is_limot = [](int unit) { return unit == UNIT_LIMOT || unit == UNIT_SLIMOT || unit == UNIT_AMOTOR; };
    // the coefficient of friction row r (1 or 2) of a contact joint: mu_1 = max(mu, 0); mu_2 = max(surface.mu2, 0) where the caller
    // came with surfaces (dmxBatchStepJointsSurface) and the joint's mode has DMX_CONTACT_MU2, else mu_1 (include/dmx_batch.h).
    // Row count, island building and the rows that can never clamp depend on these two alone.
    const double inf_d = __builtin_huge_val();
    // (taken as the device will hold them, rounded to the batch's precision: a positive coefficient below float's smallest is 0 there
    //  too, so the host and the device count the same rows)
    auto mu_row = [&](const dmxContactJoint &j, int r) {
        double m = j.mu;
        if (r == 2 && surfaces && (j.mode & DMX_CONTACT_MU2)) m = surfaces[&j - joints].mu2;
        m = (double)(T)m;
        return m > 0 ? m : 0.0;
    };
    // (without surfaces -- dmxBatchStepJoints and the ticks that find their own contacts -- all of it is the one test of mu it was)
    auto rpc_of = [&](const CJ &c) {
        if (c.unit) return (c.unit == UNIT_HINGE2 || c.unit == UNIT_SLIDER2) ? 2 : is_limot(c.unit) ? 1 : 3;
        if (!surfaces) return c.j->mu > 0 ? 3 : 1;
        return (mu_row(*c.j, 1) > 0 || mu_row(*c.j, 2) > 0) ? 3 : 1;
    };
    auto nbd_rows_of = [&](const CJ &c) {
        if (c.unit) return is_limot(c.unit) ? 1 : 0;
        if (!surfaces) return (c.j->mu > 0 && c.j->mu < inf_d) ? 3 : 1;
        const double m1 = mu_row(*c.j, 1), m2 = mu_row(*c.j, 2);
        return (m1 > 0 || m2 > 0) ? 1 + (m1 < inf_d ? 1 : 0) + (m2 < inf_d ? 1 : 0) : 1;
    };
    // pyramid rows (DMX_CONTACT_APPROX1): friction row d of a contact whose mode has bit APPROX1_d and whose mu_d is positive and finite.
    // A tick that has one launches the kernels' APX instantiations; a tick without one launches what it launched before they existed.
    auto pyramid_bits = [&](const dmxContactJoint &j) {
        if (!surfaces) return (j.mu > 0 && j.mu < inf_d) ? (j.mode & DMX_CONTACT_APPROX1) : 0;
        const double m1 = mu_row(j, 1), m2 = mu_row(j, 2);
        return ((m1 > 0 && m1 < inf_d) ? (j.mode & DMX_CONTACT_APPROX1_1) : 0) | ((m2 > 0 && m2 < inf_d) ? (j.mode & DMX_CONTACT_APPROX1_2) : 0);
    };
    bool pyramid = false;
    // an extended tick: some contact that survives brings a bit of DMX_CONTACT_SURFACE_EXT along with its surface.  It takes the APX
    // instantiations too, and stages EXT_REALS more reals per entry (IslandSet::cext); every other tick does neither.
    auto extended_bits = [&](const dmxContactJoint &j) { return surfaces ? (j.mode & DMX_CONTACT_SURFACE_EXT) : 0; };
    bool extended = false;
    for (int64_t k = 0; k < nj_in; k++) {
        const dmxContactJoint &j = joints[k];
        int b1 = live(j.body1) ? j.body1 : -1, b2 = live(j.body2) ? j.body2 : -1;
        bool rev = false;
        if (b1 < 0 && b2 >= 0) { b1 = b2; b2 = -1; rev = true; }   // dJointAttach(c, 0, body): swap + reverse
        if (b1 < 0) continue;                                       // static-static: the stepper ignores it
        if (b1 == b2) continue;
        DmxCanonicalJoint c; c.b1 = b1; c.b2 = b2; c.j = &j; c.rev = rev;
        cj.push_back(c);
        if (pyramid_bits(j)) pyramid = true;
        if (extended_bits(j)) extended = true;
    }
    // ---- auto-disable: an island without an awake body is left out of the tick, whole; in an awake island every member is awake.
    // Only while some live slot is asleep: a batch without one does nothing here but compare a count.
    std::vector<int> &ad_dropped = b->sc_ad_dropped;        // the live slots this tick leaves out
    ad_dropped.clear();
    b->ad_skipped = 0;
    if (b->ad_n_disabled > 0 && !include && !geo) {
        UnionFind uf(b->sc_parent);
        for (const CJ &c : cj) if (c.b2 >= 0) uf.unite(c.b1, c.b2);
        for (const std::pair<int, int> &l : am_links) uf.unite(l.first, l.second);
        std::vector<uint8_t> &awake = b->sc_awake;
        awake.assign((size_t)n, 0);
        for (int s = 0; s < n; s++) if (live(s) && !(b->h_bflags[(size_t)s] & BF_DISABLED)) awake[(size_t)uf.find(s)] = 1;
        int64_t woke_lo = -1, woke_hi = -1;
        for (int s = 0; s < n; s++) {
            if (!live(s)) continue;
            const int r = uf.find(s);
            if (!awake[(size_t)r]) { ad_dropped.push_back(s); if (r == s) b->ad_skipped++; continue; }
            if (b->h_bflags[(size_t)s] & BF_DISABLED) {      // woken by the island rule: the bit goes, the counters stand
                b->h_bflags[(size_t)s] &= (uint8_t)~BF_DISABLED;
                b->ad_woken++; b->ad_n_disabled--;
                if (woke_lo < 0) woke_lo = s;
                woke_hi = s;
            }
        }
        if (!ad_dropped.empty()) {
            // their joints make no rows: the entries go before anything is counted, scheduled or staged (order kept: units first)
            size_t keep = 0;
            n_units = 0; n_limots = 0; n_amotor_rows = 0; pyramid = false; extended = false;
            {
                size_t lk = 0;
                for (const std::pair<int, int> &l : am_links) if (awake[(size_t)uf.find(l.first)]) am_links[lk++] = l;
                am_links.resize(lk);
            }
            for (size_t k = 0; k < cj.size(); k++) {
                const CJ &c = cj[k];
                if (!awake[(size_t)uf.find(c.b1)]) continue;
                if (c.unit) { n_units++; if (is_limot(c.unit)) n_limots++; if (c.unit == UNIT_AMOTOR) n_amotor_rows++; }
                else { if (pyramid_bits(*c.j)) pyramid = true; if (extended_bits(*c.j)) extended = true; }
                cj[keep++] = c;
            }
            cj.resize(keep);
        }
        // scratch back to its idle state (the tick's own grouping below starts from the identity again, over the entries kept);
        // sc_awake: 2 marks a slot left out until the tick's list of slots is made, 0 otherwise
        for (int s = 0; s < n; s++) if (live(s)) { b->sc_parent[(size_t)s] = s; awake[(size_t)s] = 0; }
        for (int s : ad_dropped) awake[(size_t)s] = 2;
        if (woke_lo >= 0) {
            b->state_version++;
            HIP_TRY(hipMemcpyAsync(b->bflags + woke_lo, b->h_bflags.data() + woke_lo, (size_t)(woke_hi - woke_lo + 1), hipMemcpyHostToDevice, b->stream));
        }
    }
    const int nc = (int)cj.size();
    if (pyramid && b->row_order_ode && !exact) {
        // ODE moves such rows to the end of its order; this library defines them in creation order only (include/dmx_batch.h)
        fprintf(stderr, "libode_mi355: dmxBatchStepJoints under DMX_ORDER_ODE with QuickStep does not honour friction bounded by the normal force "
                        "(DMX_CONTACT_APPROX1): use DMX_ORDER_CREATION\n");
        b->fb_valid = fb_was_valid;
        return DMX_EINVAL;
    }
    if (pyramid && (include || geo)) {          // (the ticks that find their own contacts refuse such a batch surface before they get here)
        fprintf(stderr, "libode_mi355: a tick of a subset of the bodies does not honour DMX_CONTACT_APPROX1\n");
        b->fb_valid = fb_was_valid;
        return DMX_EINVAL;
    }
    if (extended && b->row_order_ode && !exact) {
        fprintf(stderr, "libode_mi355: dmxBatchStepJointsSurface under DMX_ORDER_ODE with QuickStep does not honour mu2, fdir1, motion or slip "
                        "(DMX_CONTACT_SURFACE_EXT): use DMX_ORDER_CREATION\n");
        b->fb_valid = fb_was_valid;
        return DMX_EINVAL;
    }
    // (a guard only: no caller that steps a subset comes with surfaces -- dmxBatchStepJointsSurface alone passes them, with neither
    //  `include` nor `geo` -- so this refusal cannot be reached through the public interface, and has no test for that reason)
    if (extended && (include || geo)) {
        fprintf(stderr, "libode_mi355: a tick of a subset of the bodies does not honour mu2, fdir1, motion or slip (DMX_CONTACT_SURFACE_EXT)\n");
        b->fb_valid = fb_was_valid;
        return DMX_EINVAL;
    }
    const bool apx = pyramid || extended;       // the kernels' APX instantiations: a tick whose contacts carry more than box friction

    // ---- the bodies this tick steps, ascending: the caller's subset (`include`, with its list) or every live slot ----
    std::vector<int> &slots = b->sc_slots;
    slots.clear();
    if (include && b->sc_include_list) slots.assign(b->sc_include_list, b->sc_include_list + b->sc_include_count);
    else if (ad_dropped.empty()) { for (int s = 0; s < n; s++) if (live(s)) slots.push_back(s); }
    else {
        for (int s = 0; s < n; s++) if (live(s) && b->sc_awake[(size_t)s] != 2) slots.push_back(s);
        for (int s : ad_dropped) b->sc_awake[(size_t)s] = 0;
    }
    const int nlive = (int)slots.size();
    // does the tick step a body that can fall asleep?  Then the end-of-tick rule runs behind it, and its flags travel to the host
    bool ad_tick = false;
    if (b->ad_n_auto > 0 && !include && !geo)
        for (int s : slots) if (b->h_bflags[(size_t)s] & BF_AUTODISABLE) { ad_tick = true; break; }
    const IdleParams<T> ad_params = make_idle_params<T>(b->ad_lin, b->ad_ang, b->ad_steps, b->ad_time, h);

    // ---- islands ----------------------------------------------------------------------------------------
    UnionFind uf(b->sc_parent);
    for (const CJ &c : cj) if (c.b2 >= 0) uf.unite(c.b1, c.b2);
    for (const std::pair<int, int> &l : am_links) uf.unite(l.first, l.second);
    std::vector<int> &island_of = b->sc_island;
    int ni = 0;
    for (int s : slots) {
        const int r = uf.find(s);             // roots are the lowest slot of their component
        if (r == s) island_of[(size_t)s] = ni++;
    }
    for (int s : slots)
        if (island_of[(size_t)s] < 0) island_of[(size_t)s] = island_of[(size_t)uf.find(s)];

    ph.reset(new DmxPhase(b, 5));
    // ---- which islands are large enough for a workgroup, and their level schedules (integers only) ------------
    // contacts are not yet in island order here; gather per-island contact lists in creation order first
    std::vector<int> &con_start = b->sc_iv[0];
    con_start.assign((size_t)ni + 1, 0);
    for (const CJ &c : cj) con_start[(size_t)island_of[(size_t)c.b1] + 1]++;
    for (int i = 0; i < ni; i++) con_start[(size_t)i + 1] += con_start[(size_t)i];
    std::vector<int> &con_sorted = b->sc_iv[1];          // cj indices grouped by island, creation order inside
    con_sorted.resize((size_t)nc);
    {
        std::vector<int> &f = b->sc_iv[15];
        f.assign(con_start.begin(), con_start.end() - 1);
        for (int k = 0; k < nc; k++) con_sorted[(size_t)f[(size_t)island_of[(size_t)cj[(size_t)k].b1]]++] = k;
    }
    // ---- ODE's own row order (dmxBatchSetRowOrder): within an island ODE numbers the rows in the order its island builder
    // discovers the joints -- a depth-first walk from the newest body, each body's joint list newest first [ODE-recall
    // dxProcessIslands, head-inserted lists] -- and QuickStep re-shuffles that order with the global LCG at every 8th
    // sweep (RANDOMLY_REORDER_CONSTRAINTS).  The LCG is consumed island by island in the walk's order, so the walk is
    // replayed here; the shuffled orders are made below, once the islands' row counts are known.
    const bool ode_order = b->row_order_ode && !exact;
    std::vector<int> &proc = b->sc_ode_proc;          // islands in the order ODE steps them
    proc.clear();
    if (ode_order) {
        std::vector<int> &adj_off = b->sc_ode_iv[0], &adj = b->sc_ode_iv[1], &fill = b->sc_ode_iv[2], &stack = b->sc_ode_iv[3];
        std::vector<uint8_t> &tag_b = b->sc_ode_tag_b, &tag_j = b->sc_ode_tag_j;
        adj_off.assign((size_t)n + 1, 0);
        for (const CJ &c : cj) { adj_off[(size_t)c.b1 + 1]++; if (c.b2 >= 0) adj_off[(size_t)c.b2 + 1]++; }
        for (int s = 0; s < n; s++) adj_off[(size_t)s + 1] += adj_off[(size_t)s];
        adj.resize((size_t)adj_off[(size_t)n] + 1);
        fill.assign(adj_off.begin(), adj_off.end() - 1);
        for (int k = 0; k < nc; k++) {
            adj[(size_t)fill[(size_t)cj[(size_t)k].b1]++] = k;
            if (cj[(size_t)k].b2 >= 0) adj[(size_t)fill[(size_t)cj[(size_t)k].b2]++] = k;
        }
        tag_b.assign((size_t)n, 0); tag_j.assign((size_t)nc + 1, 0);
        stack.clear();
        for (int q = nlive - 1; q >= 0; q--) {
            const int bb = slots[(size_t)q];
            if (tag_b[(size_t)bb]) continue;
            tag_b[(size_t)bb] = 1;
            const int isl = island_of[(size_t)bb];
            int at = con_start[(size_t)isl];
            int body = bb;
            for (;;) {
                const int lo = adj_off[(size_t)body], hi = adj_off[(size_t)body + 1];
                for (int t = 0; t < hi - lo; t++) {
                    const int j = adj[(size_t)(hi - 1 - t)];
                    if (tag_j[(size_t)j]) continue;
                    tag_j[(size_t)j] = 1;
                    con_sorted[(size_t)at++] = j;
                    const int other = cj[(size_t)j].b1 == body ? cj[(size_t)j].b2 : cj[(size_t)j].b1;
                    if (other >= 0 && !tag_b[(size_t)other]) { tag_b[(size_t)other] = 1; stack.push_back(other); }
                }
                if (stack.empty()) break;
                body = stack.back(); stack.pop_back();
            }
            proc.push_back(isl);
        }
    }
    std::vector<int> &crow_h = b->sc_iv[2];           // island-relative first row of each (sorted) contact
    crow_h.assign((size_t)nc, 0);
    std::vector<int> &big_h = b->sc_iv[3], &big_list_h = b->sc_iv[4], &lev_count_h = b->sc_iv[5], &lev_off_h = b->sc_iv[6],
                     &lev_rows_h = b->sc_iv[7], &lvl_all = b->sc_iv[8];
    big_h.assign((size_t)ni, -1); big_list_h.clear(); lev_count_h.clear(); lev_off_h.clear(); lev_rows_h.clear(); lvl_all.clear();
    int big_max_bodies = 0, big_max_width = 0, big_rows_total = 0, big_max_rows = 0;
    std::vector<int> &grid_list = b->sc_grid_list;      // dWorldStep: islands for the grid-wide exact solve
    grid_list.clear();
    size_t lds_need = 0;                                // ... and what the largest of the others needs of a workgroup's LDS
    std::vector<int> &island_bodies = b->sc_iv[9];
    island_bodies.assign((size_t)ni, 0);
    for (int s : slots) island_bodies[(size_t)island_of[(size_t)s]]++;
    {
        // Islands are independent, so every per-island pass below is spread over the host's cores (dmx_parallel_for).
        // (1) rows per island and each contact's first row
        std::vector<int> &m_of = b->sc_iv[10];
        std::vector<int> &nbd_of = b->sc_nbd_of;        // rows of the island that can clamp (normal rows, friction rows with finite mu)
        m_of.assign((size_t)ni, 0);
        nbd_of.assign((size_t)ni, 0);
        dmx_parallel_for(ni, 512, [&](int64_t lo, int64_t hi, int) {
            for (int64_t i = lo; i < hi; i++) {
                int m = 0, nbd = 0;
                for (int d = con_start[(size_t)i]; d < con_start[(size_t)i + 1]; d++) {
                    crow_h[(size_t)d] = m;
                    const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                    m += rpc_of(c);
                    nbd += nbd_rows_of(c);
                }
                m_of[(size_t)i] = m;
                nbd_of[(size_t)i] = nbd;
            }
        });
        // (2) the islands that get a workgroup, and where their rows sit in the flat arrays
        std::vector<int> &row_base = b->sc_iv[11];
        row_base.clear();
        int rows_total = 0;
        if (exact)
            for (int i = 0; i < ni; i++)
                if (m_of[(size_t)i] > lcp_max_exact_rows()) {
                    static bool warned = false;
                    if (!warned) fprintf(stderr, "libode_mi355: dWorldStep: an island of %d constraint rows exceeds the exact solver's limit (%d); "
                                                 "such ticks are stepped with QuickStep's SOR instead\n", m_of[(size_t)i], lcp_max_exact_rows());
                    warned = true;
                    exact = false;
                    lcp_grid_count_fallback(b);
                    break;
                }
        for (int i = 0; i < ni; i++) {
            if (ode_order) break;                     // shuffled sweeps are sequential: every island takes solve_islands
            if (m_of[(size_t)i] < (exact ? 1 : big_island_rows())) continue;
            // one body with 1..8 contacts: solve_singles' / solve_singles_lds' island (one lane), never a workgroup's
            // (not with an articulation unit -- a body on a joint to the world: those forms know contacts only; units come first)
            if (!exact && island_bodies[(size_t)i] == 1 && con_start[(size_t)i + 1] - con_start[(size_t)i] <= 8 &&
                !cj[(size_t)con_sorted[(size_t)con_start[(size_t)i]]].unit) continue;
            // dWorldStep, an island of hundreds of rows or more: the grid-wide solve (dmx_lcp.hip), not one workgroup
            // (small and medium ones: one workgroup, the whole solve in LDS, while it fits)
            if (exact && !lcp_lds_fits((int)sizeof(T), m_of[(size_t)i], nbd_of[(size_t)i])) { grid_list.push_back(i); continue; }
            if (exact && m_of[(size_t)i] >= lcp_grid_threshold()) { grid_list.push_back(i); continue; }
            if (exact) lds_need = std::max(lds_need, lcp_lds_need((int)sizeof(T), m_of[(size_t)i], nbd_of[(size_t)i]));
            big_list_h.push_back(i);
            row_base.push_back(rows_total);
            rows_total += m_of[(size_t)i];
            big_max_bodies = std::max(big_max_bodies, island_bodies[(size_t)i]);
            big_max_rows = std::max(big_max_rows, m_of[(size_t)i]);
        }
        const int nbig = (int)big_list_h.size();
        if (exact) {
            // no level schedules: the exact solve is not a sweep
            lev_count_h.assign((size_t)nbig, 0);
            for (int k = 0; k < nbig; k++) big_h[(size_t)big_list_h[(size_t)k]] = 0;
            for (int i : grid_list) big_h[(size_t)i] = 0;         // (not the lane-per-island kernel's either)
            rows_total = 0;
        }
        const int nbig_sched = exact ? 0 : nbig;
        // (3) row r's level = 1 + the latest level of an earlier row sharing a body with it (creation order)
        std::vector<int> &lvl = lvl_all;                // row -> level, laid out like lev_rows (island k's rows from row_base[k])
        lvl.assign((size_t)rows_total, 0);
        big_rows_total = rows_total;
        lev_count_h.assign((size_t)nbig, 0);
        std::vector<int> &last = b->sc_last;          // per slot: level of the latest row touching the body; islands own disjoint slots
        dmx_parallel_for(nbig_sched, 64, [&](int64_t lo, int64_t hi, int) {
            for (int64_t k = lo; k < hi; k++) {
                const int i = big_list_h[(size_t)k];
                int *lv_out = lvl.data() + row_base[(size_t)k];
                int nlev = 0, r = 0;
                for (int d = con_start[(size_t)i]; d < con_start[(size_t)i + 1]; d++) {
                    const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                    const int rpc = rpc_of(c);
                    for (int q = 0; q < rpc; q++, r++) {
                        int lv = last[(size_t)c.b1];
                        if (c.b2 >= 0 && last[(size_t)c.b2] > lv) lv = last[(size_t)c.b2];
                        lv += 1;
                        lv_out[r] = lv;
                        last[(size_t)c.b1] = lv;
                        if (c.b2 >= 0) last[(size_t)c.b2] = lv;
                        if (lv + 1 > nlev) nlev = lv + 1;
                    }
                }
                for (int d = con_start[(size_t)i]; d < con_start[(size_t)i + 1]; d++) {      // back to the idle state
                    const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                    last[(size_t)c.b1] = -1;
                    if (c.b2 >= 0) last[(size_t)c.b2] = -1;
                }
                lev_count_h[(size_t)k] = nlev;
            }
        });
        // (4) offsets of every island's level table, then (5) its rows grouped by level (counting sort)
        std::vector<int> &off_base = b->sc_iv[12];
        off_base.assign((size_t)nbig + 1, 0);
        for (int k = 0; k < nbig_sched; k++) off_base[(size_t)k + 1] = off_base[(size_t)k] + lev_count_h[(size_t)k] + 1;
        lev_off_h.assign((size_t)off_base[(size_t)nbig_sched], 0);
        lev_rows_h.assign((size_t)rows_total, 0);
        std::vector<int> &width_of = b->sc_iv[13];
        width_of.assign((size_t)nbig, 0);
        dmx_parallel_for(nbig_sched, 64, [&](int64_t lo, int64_t hi, int) {
            std::vector<int> fill;
            for (int64_t k = lo; k < hi; k++) {
                const int i = big_list_h[(size_t)k], m = m_of[(size_t)i], nlev = lev_count_h[(size_t)k], base = row_base[(size_t)k];
                int *off = lev_off_h.data() + off_base[(size_t)k];          // [nlev + 1], absolute positions in lev_rows
                const int *lv = lvl.data() + base;
                for (int q = 0; q < m; q++) off[lv[q] + 1]++;
                int w = 0;
                for (int q = 1; q <= nlev; q++) w = std::max(w, off[q]);
                width_of[(size_t)k] = w;
                off[0] = base;
                for (int q = 0; q < nlev; q++) off[q + 1] += off[q];
                fill.assign(off, off + nlev);
                for (int q = 0; q < m; q++) lev_rows_h[(size_t)fill[(size_t)lv[q]]++] = q;
            }
        });
        for (int k = 0; k < nbig_sched; k++) {
            big_h[(size_t)big_list_h[(size_t)k]] = off_base[(size_t)k];
            big_max_width = std::max(big_max_width, width_of[(size_t)k]);
        }
    }
    const int n_big = (int)big_list_h.size();
    ph.reset(new DmxPhase(b, 6));

    // ---- the single-launch tick (dmx_small.hip)?  Decided on integers the host has by now; one reason that says no sends the
    // whole tick down the general path.  The tables built above are what both paths consume.
    int why = -1;
    if (b->small_mode != DMX_SMALL_TICK_AUTO) why = DMX_SMALL_TICK_STAT_MODE;
    else if (ode_order) why = DMX_SMALL_TICK_STAT_ROW_ORDER;
    else if (include || geo) why = DMX_SMALL_TICK_STAT_SUBSET;
    else if (nlive > SMALL_MAX_BODIES || n > 8 * SMALL_MAX_BODIES) why = DMX_SMALL_TICK_STAT_BODIES;      // (the mirror and its fill cover the capacity)
    else if (ni > SMALL_MAX_ISLANDS) why = DMX_SMALL_TICK_STAT_ISLANDS;
    else if (!exact && big_max_rows > WAVE_ISLAND_ROWS) why = DMX_SMALL_TICK_STAT_SOR_ROWS;            // (the one-wavefront form of solve_island_wg)
    else if (exact && !grid_list.empty()) why = DMX_SMALL_TICK_STAT_LDS_FIT;
    else if (exact && apx) why = DMX_SMALL_TICK_STAT_LDS_FIT;      // (dWorldStep's two passes, and its APX rows: the general path's kernels only)
    const bool small = why < 0;
    b->small_stats[small ? DMX_SMALL_TICK_STAT_SMALL : DMX_SMALL_TICK_STAT_GENERAL]++;
    if (!small) b->small_stats[why]++;

    // int staging: body_off[ni+1] bodies[nlive] con_off[ni+1] row_off[ni+1] cb1[nc] cb2[nc] cmode[nc] csrc[nc] crow[nc]
    //              big[ni] big_list[n_big] lev_count[n_big] lev_off[..] lev_rows[..]
    const size_t n_int_tables = (size_t)3 * (ni + 1) + (size_t)nlive + (size_t)5 * nc + (size_t)ni + (size_t)2 * n_big +
                                lev_off_h.size() + 2 * lev_rows_h.size() +      // ... lev_rows[..] row_level[..]
                                (fb ? (size_t)3 * nc : 0);                     // feedback: fb_out[nc] fb_info[nc] fb_isl[nc]
    // a tick with an AMotor row: amotor_prepare's records behind them, one per joint of the set, at an even index (they hold doubles)
    const size_t am_nj = n_amotor_rows > 0 ? b->art.size() : 0;
    const size_t am_at = (n_int_tables + 1) & ~(size_t)1;
    const size_t n_int = am_nj ? am_at + am_nj * (sizeof(AMotorIn) / sizeof(int)) : n_int_tables;
    // feedback: 12 reals per joint of the set and per contact joint given; a small tick keeps them behind its tables' reals
    const size_t n_fb = fb ? (size_t)12 * (b->art.size() + (size_t)nj_in) : 0;
    // real staging: cpos[3nc] cnormal[3nc] cdepth cmu cbounce cbounce_vel csoft_erp csoft_cfm [nc each]
    //               and in an extended tick cext[EXT_REALS nc] behind them
    const size_t n_real = (size_t)(extended ? 12 + EXT_REALS : 12) * nc;
    int rc;
    int *hi; T *hr;
    const int sp = b->sm_parity;
    const size_t sm_real_at = ((n_int * sizeof(int) + 64 + 255) / 256) * 256;      // the reals' offset in a small tick's staging buffer
    const size_t sm_fb_at = ((sm_real_at + n_real * sizeof(T) + 64 + 255) / 256) * 256;      // ... and the feedback's, when it is on
    if (small) {
        // host-mapped staging buffer `sp`: last read by the small tick before the previous one
        if (b->sm_ev_pending[sp]) { HIP_TRY(hipEventSynchronize(b->sm_ev[sp])); b->sm_ev_pending[sp] = false; }
        if ((rc = ensure_mapped(&b->sm_stage[sp], &b->sm_stage_dev[sp], &b->sm_stage_bytes[sp], fb ? sm_fb_at + n_fb * sizeof(T) + 64 : sm_real_at + n_real * sizeof(T) + 64)) != DMX_OK) return rc;
        hi = (int *)b->sm_stage[sp];
        hr = (T *)((char *)b->sm_stage[sp] + sm_real_at);
        // the general path's own pinned staging keeps pace with the world (a compare per tick while it is large enough): a tick
        // that falls back -- one island past a limit -- must not meet its first allocations there, a millisecond of them
        if (n_int * sizeof(int) + 64 > b->jh_int_bytes || n_real * sizeof(T) + 64 > b->jh_real_bytes) {
            HIP_TRY(hipStreamSynchronize(b->stream));          // (an earlier general tick's copies may still read the old buffers)
            if ((rc = ensure_pinned(&b->jh_int, &b->jh_int_bytes, n_int * sizeof(int) + 64)) != DMX_OK) return rc;
            if ((rc = ensure_pinned(&b->jh_real, &b->jh_real_bytes, n_real * sizeof(T) + 64)) != DMX_OK) return rc;
        }
    } else {
        // previous tick's async copies read the pinned staging buffers: drain before refilling
        HIP_TRY(hipStreamSynchronize(b->stream));
        if ((rc = ensure_pinned(&b->jh_int, &b->jh_int_bytes, n_int * sizeof(int) + 64)) != DMX_OK) return rc;
        if ((rc = ensure_pinned(&b->jh_real, &b->jh_real_bytes, n_real * sizeof(T) + 64)) != DMX_OK) return rc;
        hi = (int *)b->jh_int;
        hr = (T *)b->jh_real;
    }
    int *body_off = hi, *bodies = body_off + (ni + 1), *con_off = bodies + nlive, *row_off = con_off + (ni + 1);
    int *cb1 = row_off + (ni + 1), *cb2 = cb1 + nc, *cmode = cb2 + nc, *csrc = cmode + nc, *crow = csrc + nc;
    int *big = crow + nc, *big_list = big + ni, *lev_count = big_list + n_big, *lev_off = lev_count + n_big;
    int *lev_rows = lev_off + lev_off_h.size();
    int *fb_out = lev_rows + 2 * lev_rows_h.size(), *fb_info = fb_out + nc, *fb_isl = fb_info + nc;      // (feedback on only)
    if (am_nj) dmx_amotor_records(b, (AMotorIn *)(hi + am_at));
    if (nc) memcpy(crow, crow_h.data(), (size_t)nc * sizeof(int));
    if (ni) memcpy(big, big_h.data(), (size_t)ni * sizeof(int));
    if (n_big) { memcpy(big_list, big_list_h.data(), (size_t)n_big * sizeof(int)); memcpy(lev_count, lev_count_h.data(), (size_t)n_big * sizeof(int)); }
    if (!lev_off_h.empty()) memcpy(lev_off, lev_off_h.data(), lev_off_h.size() * sizeof(int));
    if (!lev_rows_h.empty()) {
        memcpy(lev_rows, lev_rows_h.data(), lev_rows_h.size() * sizeof(int));
        memcpy(lev_rows + lev_rows_h.size(), lvl_all.data(), lev_rows_h.size() * sizeof(int));      // row_level, same layout
    }
    T *cpos = hr, *cnormal = cpos + 3 * (size_t)nc, *cdepth = cnormal + 3 * (size_t)nc, *cmu = cdepth + nc,
      *cbounce = cmu + nc, *cbv = cbounce + nc, *cserp = cbv + nc, *cscfm = cserp + nc, *cext = extended ? cscfm + nc : nullptr;

    // a slider's limot entry reads its anchors from the entry before it, which must be its own joint's linear unit: units are
    // emitted back to back and the sort by island is stable (and the ODE row order, which is not, is refused with joints set)
    if (n_limots)
        for (int d = 0; d < nc; d++) {
            const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
            if (c.unit != UNIT_SLIMOT) continue;
            const CJ *before = d > 0 ? &cj[(size_t)con_sorted[(size_t)d - 1]] : nullptr;
            if (!before || before->unit != UNIT_SLIDER2 || before->art != c.art || crow_h[(size_t)d] != crow_h[(size_t)d - 1] + 2) {
                fprintf(stderr, "libode_mi355: internal error: a slider's limit / motor unit does not follow its linear unit\n");
                for (int s : slots) { b->sc_parent[(size_t)s] = s; island_of[(size_t)s] = -1; }     // scratch back to its idle state
                return DMX_EINVAL;
            }
        }
    // counting sort of bodies and joints by island (stable: ascending slots / creation order)
    memset(body_off, 0, (size_t)(ni + 1) * sizeof(int));
    memset(con_off, 0, (size_t)(ni + 1) * sizeof(int));
    for (int s : slots) body_off[island_of[(size_t)s] + 1]++;
    for (const CJ &c : cj) con_off[island_of[(size_t)c.b1] + 1]++;
    for (int i = 0; i < ni; i++) { body_off[i + 1] += body_off[i]; con_off[i + 1] += con_off[i]; }
    for (int i = 0; i <= ni; i++) row_off[i] = 3 * con_off[i];
    {
        std::vector<int> &fill = b->sc_iv[14];
        fill.assign(body_off, body_off + ni);
        for (int s : slots) bodies[fill[(size_t)island_of[(size_t)s]]++] = s;
        // contact d of the island-ordered arrays is joint con_sorted[d] (stable counting sort above): fill in parallel
        dmx_parallel_for(nc, 8192, [&](int64_t lo, int64_t hi, int) {
            for (int64_t d = lo; d < hi; d++) {
                const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                if (cext) for (int k = 0; k < EXT_REALS; k++) cext[(size_t)EXT_REALS * (size_t)d + k] = T(0);      // (a unit's are never read)
                if (c.unit) {
                    // a unit's six reals ride in the contact arrays: the first side's anchor (axis) where a contact has its
                    // position, the second side's where it has its normal; cmu says which unit it is
                    const dmxJoint &a = b->art[(size_t)c.art];
                    if (c.unit == UNIT_LIMOT) {
                        // the limot unit: axis1 AS GIVEN where a contact has its position, the zero pose in the normal's three
                        // slots and the depth's, stops / vel / fmax in the four surface slots; cmode says whether the sides were exchanged
                        const dmxHingeLimot &l = b->limot[(size_t)c.art];
                        cb1[d] = c.b1; cb2[d] = c.b2; cmode[d] = c.rev ? 1 : 0; csrc[d] = 0;
                        for (int k = 0; k < 3; k++) { cpos[3 * (size_t)d + k] = (T)a.axis1[k]; cnormal[3 * (size_t)d + k] = (T)l.qrel0[k]; }
                        cdepth[d] = (T)l.qrel0[3]; cmu[d] = (T)UNIT_LIMOT_MU;
                        cbounce[d] = (T)l.lo_stop; cbv[d] = (T)l.hi_stop; cserp[d] = (T)l.vel; cscfm[d] = (T)l.fmax;
                        continue;
                    }
                    if (c.unit == UNIT_SLIMOT) {
                        // a slider's limot unit: axis1 AS GIVEN, stops / vel / fmax, cmode as the hinge's; its anchors are the linear
                        // unit's, the entry before it (a joint's units are emitted back to back and the sort by island is stable)
                        const dmxHingeLimot &l = b->limot[(size_t)c.art];
                        cb1[d] = c.b1; cb2[d] = c.b2; cmode[d] = c.rev ? 1 : 0; csrc[d] = 0;
                        for (int k = 0; k < 3; k++) { cpos[3 * (size_t)d + k] = (T)a.axis1[k]; cnormal[3 * (size_t)d + k] = T(0); }
                        cdepth[d] = T(0); cmu[d] = (T)UNIT_SLIMOT_MU;
                        cbounce[d] = (T)l.lo_stop; cbv[d] = (T)l.hi_stop; cserp[d] = (T)l.vel; cscfm[d] = (T)l.fmax;
                        continue;
                    }
                    if (c.unit == UNIT_AMOTOR) {
                        // one axis of an angular motor: where its prepared reals stand in IslandSet::amotor and whether the sides
                        // were exchanged, both in cmode; nothing else is read (the stops and the motor went into the prepare pass)
                        cb1[d] = c.b1; cb2[d] = c.b2; csrc[d] = 0;
                        cmode[d] = ((AMOTOR_PREP_REALS * c.art + AMOTOR_AXIS_REALS * c.axis) << 1) | (c.rev ? 1 : 0);
                        for (int k = 0; k < 3; k++) { cpos[3 * (size_t)d + k] = T(0); cnormal[3 * (size_t)d + k] = T(0); }
                        cdepth[d] = T(0); cmu[d] = (T)UNIT_AMOTOR_MU;
                        cbounce[d] = T(0); cbv[d] = T(0); cserp[d] = T(0); cscfm[d] = T(0);
                        continue;
                    }
                    if (c.unit == UNIT_LOCK) {
                        // the zero pose in canonical sides where a contact has its normal and depth: q_0, conj(q_0) after an exchange,
                        // the identity without limots
                        double q0[4] = { 1.0, 0.0, 0.0, 0.0 };
                        if (!b->limot.empty()) for (int k = 0; k < 4; k++) q0[k] = (k > 0 && c.rev ? -1.0 : 1.0) * b->limot[(size_t)c.art].qrel0[k];
                        cb1[d] = c.b1; cb2[d] = c.b2; cmode[d] = 0; csrc[d] = 0;
                        for (int k = 0; k < 3; k++) { cpos[3 * (size_t)d + k] = T(0); cnormal[3 * (size_t)d + k] = (T)q0[k]; }
                        cdepth[d] = (T)q0[3]; cmu[d] = (T)UNIT_LOCK_MU;
                        cbounce[d] = T(0); cbv[d] = T(0); cserp[d] = T(0); cscfm[d] = T(0);
                        continue;
                    }
                    if (c.unit == UNIT_SLIDER2) {
                        // the anchors as a ball unit's, the axis of (canonical) side 1 in three of the surface slots
                        const double *f1 = c.rev ? a.anchor2 : a.anchor1, *f2 = c.rev ? a.anchor1 : a.anchor2, *ax = c.rev ? a.axis2 : a.axis1;
                        cb1[d] = c.b1; cb2[d] = c.b2; cmode[d] = 0; csrc[d] = 0;
                        for (int k = 0; k < 3; k++) { cpos[3 * (size_t)d + k] = (T)f1[k]; cnormal[3 * (size_t)d + k] = (T)f2[k]; }
                        cdepth[d] = T(0); cmu[d] = (T)UNIT_SLIDER2_MU;
                        cbounce[d] = (T)ax[0]; cbv[d] = (T)ax[1]; cserp[d] = (T)ax[2]; cscfm[d] = T(0);
                        continue;
                    }
                    const double *f1 = c.unit == UNIT_BALL ? (c.rev ? a.anchor2 : a.anchor1) : (c.rev ? a.axis2 : a.axis1);
                    const double *f2 = c.unit == UNIT_BALL ? (c.rev ? a.anchor1 : a.anchor2) : (c.rev ? a.axis1 : a.axis2);
                    cb1[d] = c.b1; cb2[d] = c.b2; cmode[d] = 0; csrc[d] = 0;
                    for (int k = 0; k < 3; k++) { cpos[3 * (size_t)d + k] = (T)f1[k]; cnormal[3 * (size_t)d + k] = (T)f2[k]; }
                    cdepth[d] = T(0); cmu[d] = (T)(c.unit == UNIT_BALL ? UNIT_BALL_MU : UNIT_HINGE2_MU);
                    cbounce[d] = T(0); cbv[d] = T(0); cserp[d] = T(0); cscfm[d] = T(0);
                    continue;
                }
                const dmxContactJoint &j = *c.j;
                // (with surfaces, bit SURF_EXT_MU1_ZERO of the staged mode is the host's own: a stray one in the caller's mode goes)
                cb1[d] = c.b1; cb2[d] = c.b2; cmode[d] = surfaces ? (j.mode & ~SURF_EXT_MU1_ZERO) : j.mode;
                csrc[d] = geo ? geo->src[(size_t)(c.j - joints)] : 0;
                for (int k = 0; k < 3; k++) {
                    cpos[3 * (size_t)d + k] = (T)j.pos[k];
                    const T nk = (T)j.normal[k];
                    cnormal[3 * (size_t)d + k] = c.rev ? -nk : nk;
                }
                cdepth[d] = (T)j.depth; cmu[d] = (T)j.mu; cbounce[d] = (T)j.bounce; cbv[d] = (T)j.bounce_vel;
                cserp[d] = (T)j.soft_erp; cscfm[d] = (T)j.soft_cfm;
                if (n_units && j.mu < 0) cmu[d] = T(0);      // (what the kernels make of it anyway; below zero marks a unit)
                if (cext) {
                    // the extended surface, resolved: what a bit selects, or what the row is without it (dmx_internal.hpp at EXT_MU2)
                    const dmxContactSurface &sf = surfaces[&j - joints];
                    T *e = cext + (size_t)EXT_REALS * (size_t)d;
                    const double m1 = mu_row(j, 1), m2 = mu_row(j, 2);
                    if (!(m1 > 0) && m2 > 0) { cmu[d] = (T)m2; cmode[d] |= SURF_EXT_MU1_ZERO; }      // (three rows wherever cmu counts them)
                    e[EXT_MU2] = (T)m2;
                    if (j.mode & DMX_CONTACT_FDIR1) for (int k = 0; k < 3; k++) e[EXT_FDIR1 + k] = (T)sf.fdir1[k];
                    if (j.mode & DMX_CONTACT_MOTION1) e[EXT_MOTION1] = (T)sf.motion1;      // (no motion changes sign where the sides were exchanged: the header's rule)
                    if (j.mode & DMX_CONTACT_MOTION2) e[EXT_MOTION2] = (T)sf.motion2;
                    if (j.mode & DMX_CONTACT_MOTIONN) e[EXT_MOTIONN] = (T)sf.motionN;
                    e[EXT_SLIP1] = (j.mode & DMX_CONTACT_SLIP1) ? (T)sf.slip1 : T(-1);
                    e[EXT_SLIP2] = (j.mode & DMX_CONTACT_SLIP2) ? (T)sf.slip2 : T(-1);
                }
            }
        });
    }

    if (fb) {
        // which entries begin a joint, how many entries it has (a joint's units are adjacent: emitted back to back, stable sort)
        // and where its result goes: the set's joints first, then the caller's contact joints in the order given
        const int n_art = (int)b->art.size();
        for (int d = 0; d < nc; d++) {
            const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
            fb_isl[d] = island_of[(size_t)c.b1];
            if (!c.unit) { fb_out[d] = n_art + (int)(c.j - joints); fb_info[d] = 2 + (c.rev ? 1 : 0); continue; }
            const bool head = d == 0 || !cj[(size_t)con_sorted[(size_t)d - 1]].unit || cj[(size_t)con_sorted[(size_t)d - 1]].art != c.art;
            fb_out[d] = -1; fb_info[d] = 0;
            if (!head) continue;
            int cnt = 1;
            while (d + cnt < nc && cj[(size_t)con_sorted[(size_t)d + cnt]].unit && cj[(size_t)con_sorted[(size_t)d + cnt]].art == c.art) cnt++;
            fb_out[d] = c.art; fb_info[d] = 2 * cnt + (c.rev ? 1 : 0);
        }
    }
    for (int s : slots) { b->sc_parent[(size_t)s] = s; island_of[(size_t)s] = -1; }     // scratch back to its idle state

    // ---- device buffers -----------------------------------------------------------------------------------
    ph.reset(new DmxPhase(b, 7));
    const size_t nrows = (size_t)3 * nc;
    // (a small tick reads neither of these two, but keeps them sized for the tick that falls back: see the pinned staging above)
    if ((rc = dmx_ensure_dev(b->jd_int, n_int * sizeof(int) + 64)) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->jd_real, n_real * sizeof(T) + 64)) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->jd_rows, (nrows + 1) * ISLAND_ROW_REALS * sizeof(T))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->jd_rowjb, (nrows + 1) * 2 * sizeof(int))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->jd_bscr, ((size_t)nlive + 1) * 28 * sizeof(T))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->jd_local, (size_t)b->stride * sizeof(int))) != DMX_OK) return rc;
    if (!small && n_int) HIP_TRY(hipMemcpyAsync(b->jd_int.p, hi, n_int * sizeof(int), hipMemcpyHostToDevice, b->stream));
    if (!small && n_real) HIP_TRY(hipMemcpyAsync(b->jd_real.p, hr, n_real * sizeof(T), hipMemcpyHostToDevice, b->stream));

    IslandSet<T> I;
    // (a small tick's kernel reads the tables where the host wrote them: the device address of the mapped staging)
    int *di = small ? (int *)b->sm_stage_dev[sp] : (int *)b->jd_int.p;
    T *dr = small ? (T *)((char *)b->sm_stage_dev[sp] + sm_real_at) : (T *)b->jd_real.p;
    I.n_islands = ni;
    I.body_off = di; I.bodies = di + (ni + 1); I.con_off = I.bodies + nlive; I.row_off = I.con_off + (ni + 1);
    I.cb1 = I.row_off + (ni + 1); I.cb2 = I.cb1 + nc; I.cmode = I.cb2 + nc;
    I.csrc = geo ? I.cmode + nc : nullptr;
    I.crow = I.cmode + 2 * (size_t)nc;
    I.big = I.crow + nc; I.n_big = n_big; I.big_list = I.big + ni; I.lev_count = I.big_list + n_big;
    I.lev_off = I.lev_count + n_big; I.lev_rows = I.lev_off + lev_off_h.size();
    I.big_max_bodies = big_max_bodies; I.big_max_width = big_max_width;
    I.big_rows_total = big_rows_total; I.big_max_rows = exact ? 0 : big_max_rows;
    I.row_level = I.lev_rows + lev_rows_h.size();
    I.gpos = geo ? (const T *)geo->pos : nullptr; I.gnormal = geo ? (const T *)geo->normal : nullptr;
    I.gdepth = geo ? (const T *)geo->depth : nullptr;
    I.cpos = dr; I.cnormal = dr + 3 * (size_t)nc; I.cdepth = I.cnormal + 3 * (size_t)nc; I.cmu = I.cdepth + nc;
    I.cbounce = I.cmu + nc; I.cbounce_vel = I.cbounce + nc; I.csoft_erp = I.cbounce_vel + nc; I.csoft_cfm = I.csoft_erp + nc;
    I.cext = extended ? I.csoft_cfm + nc : nullptr;
    I.rows = (T *)b->jd_rows.p; I.rowjb = (int *)b->jd_rowjb.p; I.bscr = (T *)b->jd_bscr.p; I.local = (int *)b->jd_local.p;
    I.singles = (exact || ode_order) ? 0 : 1;
    if (apx) I.singles = 0;      // (the one-body forms know box friction only: solve_islands' row form takes their islands, as with feedback on)
    FeedbackSet<T> F;
    if (fb) {
        // every solve must leave lambda in the row table: the one-body forms keep their rows in registers, so their islands take
        // solve_islands' row form (held bit-identical to them by tests/test_gpu_static.py and tests/test_gpu_parity.py)
        I.singles = 0;
        F.mode = exact ? FB_UNSCALED : FB_SCALED;
        F.out = di + (fb_out - hi); F.info = di + (fb_info - hi); F.isl = di + (fb_isl - hi);
        if (small) {
            T *fbh = (T *)((char *)b->sm_stage[sp] + sm_fb_at);
            for (size_t k = 0; k < n_fb; k++) fbh[k] = T(0);      // (inactive and dropped joints report zeros)
            F.fb = (T *)((char *)b->sm_stage_dev[sp] + sm_fb_at);
            b->fb_host = fbh;
        } else {
            if ((rc = dmx_ensure_dev(b->fb_dev, n_fb * sizeof(T) + 64)) != DMX_OK) return rc;
            HIP_TRY(hipMemsetAsync(b->fb_dev.p, 0, n_fb * sizeof(T) + 64, b->stream));
            F.fb = (T *)b->fb_dev.p;
            b->fb_host = nullptr;
        }
        b->fb_devp = F.fb;
        b->fb_nj = (int64_t)b->art.size(); b->fb_nc = nj_in;
    }
    I.has_units = n_units > 0 ? 1 : 0;
    b->last_units = n_units;               // (the kernels count an island's entries: dmxBatchLastContactCount takes these off)
    I.order = nullptr; I.order_stride = 0;
    if (ode_order) {
        // the shuffled row orders, one per 8 sweeps, islands in ODE's processing order (the LCG is global and sequential)
        const int epochs = (b->iters + 7) / 8;
        const size_t R = nrows + 1;
        std::vector<int> &ord_h = b->sc_ode_order, &cur = b->sc_ode_iv[0];
        ord_h.assign((size_t)std::max(epochs, 1) * R, 0);
        const std::vector<int> &m_of = b->sc_iv[10];
        for (int isl : proc) {
            const int m = m_of[(size_t)isl];
            if (m <= 0) continue;
            const size_t base = (size_t)3 * con_start[(size_t)isl];
            cur.resize((size_t)m);
            for (int q = 0; q < m; q++) cur[(size_t)q] = q;
            for (int e = 0; e < epochs; e++) {
                for (int q = 1; q < m; q++) {
                    b->ode_rand = 1664525u * b->ode_rand + 1013904223u;                 // dRand [ODE-recall misc.cpp]
                    const int sw = (int)(((uint64_t)b->ode_rand * (uint32_t)(q + 1)) >> 32);   // dRandInt(q + 1)
                    std::swap(cur[(size_t)q], cur[(size_t)sw]);
                }
                memcpy(ord_h.data() + (size_t)e * R + base, cur.data(), (size_t)m * sizeof(int));
            }
        }
        if ((rc = dmx_ensure_dev(b->jd_order, ord_h.size() * sizeof(int))) != DMX_OK) return rc;
        HIP_TRY(hipMemcpyAsync(b->jd_order.p, ord_h.data(), ord_h.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
        I.order = (const int *)b->jd_order.p; I.order_stride = (int)R;
    }

    StepParams<T> P = dmx_make_params<T>(b, h);
    // damping, angular speed cap, contact correction (include/dmx_batch.h, "damping").  The scalars ride in the island set; the
    // table reaches finish_body only while some slot's maximum speed is finite, and the damping pass goes in front of the tick's
    // first kernel -- the single-launch tick's one launch included, whose body list it reads where that launch reads it -- only
    // while some slot's scale is not zero.  (A tick of a subset comes from a caller that has refused any of this.)
    I.surface_layer = (T)b->surface_layer; I.max_corr_vel = (T)b->max_corr_vel;
    if (am_nj) {
        // the angular motors' axes and angles from the state at the tick's start: a dispatch of its own in front of the tick's first
        // kernel -- of the single-launch tick's one launch too, whose staging it reads its records from, as the damping pass does
        if ((rc = dmx_ensure_dev(b->amotor_prep, (size_t)(AMOTOR_PREP_REALS + 3) * am_nj * sizeof(T))) != DMX_OK) return rc;
        I.amotor = (const T *)b->amotor_prep.p;
        // (k as the island kernels form it: hinv * erp with hinv = 1 / h, in the batch's precision)
        HIP_TRY(launch_amotor_prepare<T>((const T *)b->slab, b->stride, (const AMotorIn *)(di + am_at), (int)am_nj, (T(1) / P.h) * P.erp,
                                         (T *)b->amotor_prep.p, (T *)nullptr, b->stream));
    }
    if (!include && !geo) {
        if (b->damp_n_capped > 0) I.damping = (const T *)b->damp_dev;
        if (b->damp_n_scaled > 0) HIP_TRY(launch_damping<T>((T *)b->slab, b->bflags, (const T *)b->damp_dev, I.bodies, nlive, n, b->stream));
    }
    if (small) {
        // one launch: islands with rows a workgroup each, free bodies and one-body islands a lane each; the new state goes to
        // the slab and to the mirror.  Nobody waits here: dmxBatchDownload(DMX_STATE) does, when the caller reads a pose.
        if (!b->sm_mirror) {
            HIP_TRY(hipHostMalloc(&b->sm_mirror, (size_t)n * C_MASS * sizeof(T) + 64, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer(&b->sm_mirror_dev, b->sm_mirror, 0));
        }
        if (exact && !b->sm_lcp_touched) {        // ... and dWorldStep's own code object (dmx_lcp.hip), which dmxBatchCreate does not load
            (void)dmx_touch_lcp((int)sizeof(T));
            b->sm_lcp_touched = true;
        }
        if (!b->sm_diag) {
            HIP_TRY(hipMalloc((void **)&b->sm_diag, 2 * sizeof(StepDiag)));
            HIP_TRY(hipMemsetAsync(b->sm_diag, 0, 2 * sizeof(StepDiag), b->stream));
        }
        if (!b->sm_ev[sp]) HIP_TRY(hipEventCreateWithFlags(&b->sm_ev[sp], hipEventDisableTiming));
        SmallTick<T> K;
        K.mirror = (T *)b->sm_mirror_dev;
        const int cur = b->sm_diag_cur ^ 1;                    // (the slot the previous small tick zeroed)
        K.diag_next = b->sm_diag + (cur ^ 1);
        K.n_slots = n;
        K.full = b->sm_mirror_valid ? 0 : 1;
        K.lds_bodies = 1; K.murty = 0; K.tol_rel = T(0);
        size_t lds;
        if (exact) {
            double tol;
            lcp_lds_knobs((int)sizeof(T), &K.murty, &tol);
            K.tol_rel = (T)tol;
            lds = lds_need;
        } else {
            lds = small_tick_sor_lds((int)sizeof(T), big_max_bodies, &K.lds_bodies);
        }
        // the kernel's AD instantiation: for the end-of-tick rule, and whenever slots were left out (a full refresh of the mirror
        // must cover them).  The flag mirror starts as the host's bytes, the slots left out marked.
        const bool ad_kernel = ad_tick || !ad_dropped.empty();
        if (ad_kernel) {
            if ((rc = dmx_ad_ensure(b)) != DMX_OK) return rc;
            memcpy(b->ad_mirror, b->h_bflags.data(), (size_t)n);
            for (int s : ad_dropped) b->ad_mirror[s] |= SMALL_AD_SKIPPED;
            K.ad_flags = b->bflags; K.ad_mirror = b->ad_mirror_dev;
            K.ad_steps = b->ad_steps_dev; K.ad_time = b->ad_time_dev; K.ad = ad_params;
        }
        HIP_TRY(launch_small_tick<T>((T *)b->slab, b->bflags, b->stride, I, P, b->sm_diag + cur, K, F, exact, lds, b->stream, apx, ad_kernel));
        HIP_TRY(hipEventRecord(b->sm_ev[sp], b->stream));
        if (ad_tick) { b->ad_wait_ev = b->sm_ev[sp]; b->ad_pending = true; }      // (the tick's own event gates the flag mirror too)
        b->sm_ev_pending[sp] = true;
        b->sm_parity = sp ^ 1;
        b->sm_diag_cur = cur;
        b->sm_mirror_valid = true;
        b->state_version++;               // (this tick wrote body state too: what rays see has moved on)
        b->last_small = true;
        b->last_islands = true;
        b->ext_pending = false;
        b->stepped_with_plane = true;     // diagnostics are valid
        b->fb_valid = fb;
        return DMX_OK;
    }
    dmx_state_written(b);
    b->last_small = false;
    HIP_TRY(hipMemsetAsync(b->diag_isl, 0, sizeof(StepDiag), b->stream));
    if (exact) {
        HIP_TRY(launch_islands_without_rows<T>((T *)b->slab, b->bflags, b->stride, I, P, b->diag_isl, b->stream));
        HIP_TRY(launch_lcp_lds<T>((T *)b->slab, b->bflags, b->stride, I, P, b->diag_isl, lds_need, b->stream, apx));
        // Written for a copy from pageable host memory that is gone; but the grid solves' host loop below and the next tick's
        // rewrite of the host staging have run behind this wait ever since, and no test tells a missing wait from a present one.
        // Taking it out is a change of speed, to be made and measured on its own.
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (!grid_list.empty()) {
            // the large islands, one after the other: per row whether it can ever clamp, and the key its active-set state is
            // remembered under -- (body pair, ordinal of the contact within the pair this tick, row of the contact)
            lcp_grid_begin_tick(b);
            LcpIslandRows R;
            R.limots = n_limots > 0;
            R.pyramid_tick = apx;
            std::vector<std::pair<uint64_t, int>> &ord = b->sc_pair_ord;
            for (int isl : grid_list) {
                R.isl = isl; R.m = b->sc_iv[10][(size_t)isl]; R.row_base = 3 * con_start[(size_t)isl];
                R.unbounded.assign((size_t)R.m, 0); R.key.assign((size_t)R.m, 0);
                R.pyramid = false; R.pyramid_row.assign((size_t)R.m, 0);
                const int d0 = con_start[(size_t)isl], d1 = con_start[(size_t)isl + 1];
                ord.clear();
                for (int d = d0; d < d1; d++) {
                    const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                    ord.push_back({ ((uint64_t)(uint32_t)(c.b1 + 1) << 32) | (uint32_t)(c.b2 + 1), d });
                }
                std::stable_sort(ord.begin(), ord.end(), [](const std::pair<uint64_t, int> &x, const std::pair<uint64_t, int> &y) { return x.first < y.first; });
                for (size_t e = 0, run = 0; e < ord.size(); e++) {
                    if (e > 0 && ord[e].first != ord[e - 1].first) run = e;
                    const int d = ord[e].second;
                    const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                    const int r = crow_h[(size_t)d], rpc = rpc_of(c);
                    const uint64_t base = ((uint64_t)(uint32_t)(c.b1 + 1) << 38) | ((uint64_t)((uint32_t)(c.b2 + 1) & 0xffffffu) << 14) |
                                          ((uint64_t)((e - run) & 0xfffu) << 2);
                    for (int q = 0; q < rpc; q++) {
                        // (a limot's row: low bits 1, as a bounded friction row's -- clamped, its value need not be zero.  The
                        //  ordinal within the pair is stable while the set and the limots' presence are)
                        R.key[(size_t)(r + q)] = base | (uint64_t)(is_limot(c.unit) ? 1 : q);
                        R.unbounded[(size_t)(r + q)] = c.unit ? !is_limot(c.unit) : (q > 0 && !((surfaces ? mu_row(*c.j, q) : c.j->mu) < inf_d));
                        if (!c.unit && q > 0 && (pyramid_bits(*c.j) & (DMX_CONTACT_APPROX1_1 << (q - 1)))) { R.pyramid_row[(size_t)(r + q)] = 1; R.pyramid = true; }
                    }
                }
                // every body's rows (creation order): counting sort over the island's contacts; local index = position among the
                // island's bodies, which are the ascending slots body_off lists
                const int ib0 = body_off[isl], inb = body_off[isl + 1] - ib0;
                std::vector<int> &loc = b->sc_last;         // (-1 outside this block)
                for (int k = 0; k < inb; k++) loc[(size_t)bodies[ib0 + k]] = k;
                R.boff.assign((size_t)inb + 1, 0);
                for (int d = d0; d < d1; d++) {
                    const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                    const int rpc = rpc_of(c);
                    R.boff[(size_t)loc[(size_t)c.b1] + 1] += rpc;
                    if (c.b2 >= 0) R.boff[(size_t)loc[(size_t)c.b2] + 1] += rpc;
                }
                for (int k = 0; k < inb; k++) R.boff[(size_t)k + 1] += R.boff[(size_t)k];
                R.bodyrows.assign((size_t)R.boff[(size_t)inb], 0);
                {
                    std::vector<int> &fill = b->sc_iv[14];
                    fill.assign(R.boff.begin(), R.boff.end() - 1);
                    for (int d = d0; d < d1; d++) {
                        const CJ &c = cj[(size_t)con_sorted[(size_t)d]];
                        const int r = crow_h[(size_t)d], rpc = rpc_of(c);
                        for (int q = 0; q < rpc; q++) {
                            R.bodyrows[(size_t)fill[(size_t)loc[(size_t)c.b1]]++] = 2 * (r + q);
                            if (c.b2 >= 0) R.bodyrows[(size_t)fill[(size_t)loc[(size_t)c.b2]]++] = 2 * (r + q) + 1;
                        }
                    }
                }
                for (int k = 0; k < inb; k++) loc[(size_t)bodies[ib0 + k]] = -1;
                if ((rc = lcp_grid_solve<T>(b, I, P, R)) != DMX_OK) return rc;
            }
            lcp_grid_end_tick(b);
            HIP_TRY(hipStreamSynchronize(b->stream));
        }
        if (fb) HIP_TRY(launch_feedback<T>(I, P, F, nc, b->stream));
    } else {
        HIP_TRY(launch_islands<T>((T *)b->slab, b->bflags, b->stride, I, P, b->diag_isl, b->stream, fb, apx));
        if (fb) HIP_TRY(launch_feedback<T>(I, P, F, nc, b->stream));
        if (ode_order) HIP_TRY(hipStreamSynchronize(b->stream));      // the order table came from pageable host memory
    }
    if (ad_tick) {
        // behind the tick's last kernel: the rule for every slot it stepped, then the flag bytes on their way to the host
        if ((rc = dmx_ad_ensure(b)) != DMX_OK) return rc;
        HIP_TRY(launch_autodisable_update<T>((T *)b->slab, b->bflags, b->ad_steps_dev, b->ad_time_dev, ad_params, I.bodies, nlive, n, b->stream));
        HIP_TRY(hipMemcpyAsync(b->ad_mirror, b->bflags, (size_t)n, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipEventRecord(b->ad_ev, b->stream));
        b->ad_wait_ev = b->ad_ev; b->ad_pending = true;
    }
    b->fb_valid = fb;
    b->last_islands = true;
    b->ext_pending = false;
    b->stepped_with_plane = true;     // diagnostics are valid
    return DMX_OK;
}

}  // namespace

int dmx_step_joints(dmxBatch *b, double h, int64_t n_joints, const dmxContactJoint *joints, const uint8_t *include,
                    const DevGeometry *geo, const dmxContactSurface *surfaces)
{
    b->fix.brk();       // the joints tick, single-launch or not, steps bodies behind the fixed-axis words' back (dmx_fixed.hpp)
    return b->precision == DMX_F32 ? step_joints_t<float>(b, h, n_joints, joints, include, geo, surfaces)
                                   : step_joints_t<double>(b, h, n_joints, joints, include, geo, surfaces);
}

extern "C" int dmxBatchStepJoints(dmxBatchID b, double h, int64_t n_joints, const dmxContactJoint *joints)
{
    if (!b || !(h > 0) || n_joints < 0 || (n_joints > 0 && !joints)) return DMX_EINVAL;
    HIP_TRY(hipSetDevice(b->device));
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    if (b->row_order_ode && !b->stepper_exact && !b->art.empty()) {      // (dWorldStep never uses the order)
        fprintf(stderr, "libode_mi355: dmxBatchStepJoints under DMX_ORDER_ODE does not honour articulation joints (dmxBatchSetJoints): "
                        "%lld are set\n", (long long)b->art.size());
        return DMX_EINVAL;
    }
    return dmx_step_joints(b, h, n_joints, joints, nullptr, nullptr);
}

// dmxBatchStepJoints with the rest of ODE's contact surface beside every joint (include/dmx_batch.h at DMX_CONTACT_MU2)
extern "C" int dmxBatchStepJointsSurface(dmxBatchID b, double h, int64_t n_joints, const dmxContactJoint *joints, const dmxContactSurface *surfaces)
{
    if (!surfaces) return dmxBatchStepJoints(b, h, n_joints, joints);
    if (!b || !(h > 0) || n_joints < 0 || (n_joints > 0 && !joints)) return DMX_EINVAL;
    // the fields the tick would read, before anything is touched -- as the device will hold them: in a float32 batch a double above
    // float's largest is an infinity there, and is refused as one
    const double inf = __builtin_huge_val();
    const bool f32 = b->precision == DMX_F32;
    auto held = [&](double x) { return f32 ? (double)(float)x : x; };
    auto finite = [&](double x) { x = held(x); return x > -inf && x < inf; };
    for (int64_t k = 0; k < n_joints; k++) {
        const int mode = joints[k].mode;
        if (!(mode & DMX_CONTACT_SURFACE_EXT)) continue;
        dmxContactSurface s = surfaces[k];
        s.slip1 = held(s.slip1); s.slip2 = held(s.slip2);
        const char *what = nullptr;
        if ((mode & DMX_CONTACT_MU2) && s.mu2 != s.mu2) what = "mu2 is NaN";
        else if ((mode & DMX_CONTACT_FDIR1) && !(finite(s.fdir1[0]) && finite(s.fdir1[1]) && finite(s.fdir1[2]))) what = "fdir1 is not finite";
        else if ((mode & DMX_CONTACT_MOTION1) && !finite(s.motion1)) what = "motion1 is not finite";
        else if ((mode & DMX_CONTACT_MOTION2) && !finite(s.motion2)) what = "motion2 is not finite";
        else if ((mode & DMX_CONTACT_MOTIONN) && !finite(s.motionN)) what = "motionN is not finite";
        else if ((mode & DMX_CONTACT_SLIP1) && !(s.slip1 >= 0 && s.slip1 < inf)) what = "slip1 is negative or not finite";
        else if ((mode & DMX_CONTACT_SLIP2) && !(s.slip2 >= 0 && s.slip2 < inf)) what = "slip2 is negative or not finite";
        if (what) {
            fprintf(stderr, "libode_mi355: dmxBatchStepJointsSurface: contact joint %lld: %s\n", (long long)k, what);
            return DMX_EINVAL;
        }
    }
    HIP_TRY(hipSetDevice(b->device));
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    if (b->row_order_ode && !b->stepper_exact && !b->art.empty()) {      // (as dmxBatchStepJoints)
        fprintf(stderr, "libode_mi355: dmxBatchStepJoints under DMX_ORDER_ODE does not honour articulation joints (dmxBatchSetJoints): "
                        "%lld are set\n", (long long)b->art.size());
        return DMX_EINVAL;
    }
    return dmx_step_joints(b, h, n_joints, joints, nullptr, nullptr, surfaces);
}
