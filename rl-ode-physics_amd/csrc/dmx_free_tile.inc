// One tile's worth of a contact-free launch: body i's loads, ticks and stores (the wavefront's 64 bodies are one tile of the slab).
// A fragment, not a header: the body of integrate_free's grid-stride loop (dmx_kernels.hip), included there and, for a wavefront that
// cannot take its straight line, in integrate_free_lean -- defined once.  Text and not a device function, because every way of
// passing the launch's arguments to a function changed the register allocation of integrate_free's 32 instantiations
// (profiles/lean_kernel_resources.txt); included, they assemble to what they were.  It expects in scope: T, the compile-time EXT, FIX,
// TF, ELIDE, UNI, NLOAD; S, So, P, fix_mode, fix_words, tf, lc, nticks, in_place, i; and an enclosing loop for its `continue`.
        if constexpr (!FIX) {
            if (P.skip != nullptr && P.skip[i]) continue;      // this body belongs to the island path this tick
        }
        T c[NLOAD];
        uint32_t fixed = 0, seen = 0;       // FIX, lean launches: the tile's word as read, and its lateral axes (wave-uniform)
        if constexpr (FIX) {
            // The tile's word first, then the loads every tile needs (pos.y, quat, lvel.y, avel and the constants): they are in flight
            // before anything waits on the word.  Only then the lateral loads, one scalar branch per axis around both of its loads.
            // The y axis is among the loads issued ahead of the word, so a fixed y saves nothing and bit 1 is kept for the record.
            uint32_t word = 0;
            if (fix_mode == FIX_LEAN) word = fix_words[__builtin_amdgcn_readfirstlane((int)(i >> 6))];
#pragma unroll
            for (int k = 0; k < NLOAD; k++)
                if (k >= C_MASS || fix_axis_of(k) < 0 || fix_axis_of(k) == 1) c[k] = S[slab_ix(k, i)];
            seen = __builtin_amdgcn_readfirstlane(word);
            fixed = seen & 5u;
#pragma unroll
            for (int ax = 0; ax < 3; ax += 2) {
                if (fixed & (1u << ax)) { c[C_POS + ax] = T(0); c[C_LVEL + ax] = T(0); }     // never looked at: see the stores
                else { c[C_POS + ax] = S[slab_ix(C_POS + ax, i)]; c[C_LVEL + ax] = S[slab_ix(C_LVEL + ax, i)]; }
            }
        } else {
#pragma unroll
            for (int k = 0; k < NLOAD; k++) c[k] = S[slab_ix(k, i)];
        }
        T was[ELIDE ? C_MASS : 1];          // the state as loaded, to tell which components the launch changed
        if constexpr (ELIDE) {
#pragma unroll
            for (int k = 0; k < C_MASS; k++) was[k] = c[k];
        }
        T bx, bz, bs;
        if (P.bp_check) { bx = S[slab_ix(C_BPX, i)]; bz = S[slab_ix(C_BPZ, i)]; bs = S[slab_ix(C_BPSAFE, i)]; }
        T f[6];
        if (EXT) {
#pragma unroll
            for (int k = 0; k < 6; k++) f[k] = S[slab_ix(C_FORCE + k, i)];
        }
        // P.ticks ticks with the state in registers: one read and one write of the state per launch, not per tick
        for (int s = 0; s < nticks; s++) {
            if (P.bp_check && ((P.bp_check & BPC_ALL) || (s == 0 && (P.bp_check & BPC_FIRST)) ||
                               (s == nticks - 1 && (P.bp_check & BPC_LAST)))) {
                // dSpaceCollide for body-body pairs, by proof: a body inside its safe zone cannot touch any other
                int z = zone_state(c[C_POS] - bx, c[C_POS + 2] - bz, bs);
                if (P.n_static > 0) {
                    const int z2 = static_state(P, c[C_POS], c[C_POS + 1], c[C_POS + 2], S[slab_ix(C_BPR, i)]);
                    z = z2 > z ? z2 : z;
                }
                report_zone(z, P.bp_flags);
            }
            V3<T> x = { c[C_POS], c[C_POS + 1], c[C_POS + 2] };
            Q4<T> q = { c[C_QUAT], c[C_QUAT + 1], c[C_QUAT + 2], c[C_QUAT + 3] };
            V3<T> v = { c[C_LVEL], c[C_LVEL + 1], c[C_LVEL + 2] };
            V3<T> w = { c[C_AVEL], c[C_AVEL + 1], c[C_AVEL + 2] };
            T mass;
            V3<T> Ib;
            if constexpr (UNI) { mass = P.uni_mass; Ib = P.uni_inertia; }
            else { mass = c[C_MASS]; Ib = { c[C_INERTIA], c[C_INERTIA + 1], c[C_INERTIA + 2] }; }
            V3<T> facc = { T(0), T(0), T(0) }, tacc = { T(0), T(0), T(0) };
            if (EXT && s == 0) {                       // the accumulators act in the first tick and are cleared by it
                facc = { f[0], f[1], f[2] };
                tacc = { f[3], f[4], f[5] };
            }
            if constexpr (UNI) {
                // what the tick makes of the launch's constants alone arrives with them (dmx_launch_consts.hpp: the quotients;
                // dmx_torque_free.hpp: hm and m g): nothing here divides, and nothing is left to compute ahead of the loop
                const TickGiven<T, EXT> K = { { lc.inv_Ib[0], lc.inv_Ib[1], lc.inv_Ib[2] }, lc.iso != 0, lc.inv_h, tf.hm, mass,
                                              { tf.mg[0], tf.mg[1], tf.mg[2] } };
                if constexpr (TF) {
                    // the short tick for a wavefront whose every active lane it is proven for, the general one for any other
                    free_body_step_torque_free(x, q, v, w, Ib, P.g, P.h, P.gyro, tf.on, K);
                } else {
                    free_body_step_with(x, q, v, w, Ib, facc, tacc, P.g, P.h, P.gyro, K);
                }
            } else {
                free_body_step(x, q, v, w, mass, Ib, facc, tacc, P.g, P.h, P.gyro);
            }
            if (s == nticks - 1) pack_boundary(P, i, x, q, v, w);
            c[C_POS] = x.x; c[C_POS + 1] = x.y; c[C_POS + 2] = x.z;
            c[C_QUAT] = q.w; c[C_QUAT + 1] = q.x; c[C_QUAT + 2] = q.y; c[C_QUAT + 3] = q.z;
            c[C_LVEL] = v.x; c[C_LVEL + 1] = v.y; c[C_LVEL + 2] = v.z;
            c[C_AVEL] = w.x; c[C_AVEL + 1] = w.y; c[C_AVEL + 2] = w.z;
        }
        if constexpr (FIX) {
            uint32_t moved = 0;             // axes on which some lane's pos or lvel changed its bits in this tick
#pragma unroll
            for (int k = 0; k < C_MASS; k++) {
                const int ax = fix_axis_of(k);
                if (ax >= 0 && (fixed & (1u << ax))) continue;      // proven fixed and not loaded: nothing to test, nothing to write
                if (in_place || ax >= 0) {
                    const bool changed = __ballot(bits_differ(c[k], was[k])) != 0ull;
                    if (ax >= 0 && changed) moved |= 1u << ax;
                    if (in_place && !changed) continue;
                }
                store_state(&So[slab_ix(k, i)], c[k]);
            }
            // what this launch observed: an establishing launch writes every tile's word, a lean one only a word that changes
            // (an axis it did not load keeps its bit: same inputs, same bits)
            const uint32_t word = ~moved & 7u;
            if ((fix_mode != FIX_LEAN || word != seen) && (threadIdx.x & 63) == 0) fix_words[i >> 6] = word;
        } else {
#pragma unroll
        for (int k = 0; k < C_MASS; k++) {
            if constexpr (ELIDE) if (in_place) {
                if (__ballot(bits_differ(c[k], was[k])) == 0ull) continue;      // all 64 bodies keep this component's bits: nothing to write
            }
            store_state(&So[slab_ix(k, i)], c[k]);       // (dmx_internal.hpp: the state leaves with the store policy's cache bit)
        }
        }
        if (EXT) {
#pragma unroll
            for (int k = 0; k < 6; k++) S[slab_ix(C_FORCE + k, i)] = T(0);
        }
