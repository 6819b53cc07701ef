// tw_env_rollout_loop.hpp -- the step loop of the device-environment PPO rollout: the BODY of rollout_env_kernel, of
// rollout_env16_kernel and of rollout_env16x2_kernel (tw_rollout_env.hpp), which include this file inside their function bodies.  NO
// once-pragma and no include guard: it is included three times, once per kernel.  It is no header of its own -- nothing else may include it.
//
// The including kernel has in scope, before the #include:
//   Env, NC    its template parameters
//   Eng        the engine: EngineV<NC>, EngineV16<NC> or EngineV16x2<NC>
//   a          an EnvRolloutArgs, by value or by const reference
//   proto      the prototype, a const Env
//   lds        the dynamic LDS (extern __shared__ float lds[], aligned to 16)
//   eng        a declared `Eng eng`; EngineV16: with eng.img already set; EngineV16x2: with eng.img and eng.err already set
//
// Shared as TEXT and not as a function template: a function that both kernels inline changed how this compiler allocates the f32
// kernels (device environments), and those stay what they are, instruction for instruction.
//
// Persistent form (a.queue != null; a kernel-argument-uniform branch, not a second instantiation): the grid holds fewer columns than
// there are episodes, and at the end of a step -- where ids and rowoff are dead -- a column whose episode is over takes the next index
// from the counter.  The writer lane draws it; it goes round to every lane of every wave that carries column j through lds_user and
// one barrier, which depends on a.queue alone (as rollout_f32_kernel does for Eng::SPLIT).  Records, ids and ep_len are addressed by
// episode, so the bytes are those of the plain launch whichever column ran an episode.
    constexpr int A = Env::NUM_ACTIONS, NO = Env::N_OBS;
    // EngineV<64> alone takes some 450 registers: a fixed-length observation of 37 .. 64 ids kept alive across the forward on top of
    // them spilled to scratch memory.  There the ids are stored BEFORE the forward, as env_rows_n stores a variable-length record's
    // (of an observation with a bad id the row is written all the same; the collect fails and nobody reads it)
    constexpr bool EARLY_IDS = NC > 36 && !EnvHasObserveN<Env>::value;
    eng.begin1(a.pol, lds);
    const int j = eng.j;
    // every lane group of every wave carries the state of column j (the engine's mapping); lanes 0-15 of wave 0 store
    const uint64_t e_first = (uint64_t)blockIdx.x * Eng::EPB + (uint64_t)j;
    const bool valid  = e_first < a.num_episodes;
    const bool writer = eng.h == 0 && eng.primary();
    uint32_t e_taken = 0xffffffffu;                                                   // the episode taken from the queue; none: e_first
    Env st = proto;
    bool alive = valid;
    bool fresh = valid;                                                               // the column's episode is still to be reset
    bool more  = valid && a.queue != nullptr;                                         // the queue may still hold episodes
    int  t = 0;
    eng.begin2();
    while (__syncthreads_or(alive ? 1 : 0)) {
        const uint64_t e_local  = e_taken != 0xffffffffu ? (uint64_t)e_taken : (uint64_t)blockIdx.x * Eng::EPB + (uint64_t)j;
        const uint64_t e_global = a.episode_offset + e_local;
        // the ONE place the struct's reset() is called from, the column's first episode and every one it takes from the queue alike
        // (with a second call site the compiler stopped inlining it, and the state went to scratch memory)
        if (fresh) {
            st = proto;                                                               // clone of the prototype (ppo.rs:59)
            st.reset(a.seed, e_global);                                               // ppo.rs:60
            fresh = false;
        }
        int perm = -1;
        if (eng.pol.n_perms > 0) {                                                    // get_perm_id (policy.rs:67-77)
            const u32x4 w = rng_draw(a.seed, e_global, (uint32_t)t, STREAM_PERM);
            perm = (int)u32_below(w.x, (uint32_t)eng.pol.n_perms);
        }
        int ids[NO], rowoff[NC];
        bool bad = false; int bad_id = 0;
        [[maybe_unused]] bool bad_count = false;                                      // (a struct with observe_n: a count outside 0 .. n_obs)
        if (alive) {
            if constexpr (EnvHasObserveN<Env>::value)
                (void)env_rows_n<Env, NC>(st, eng.pol, perm, ids, rowoff, bad, bad_id, bad_count,
                                          writer ? a.obs16 + (e_local * (uint64_t)a.out.t_pad + (uint64_t)t) * (uint64_t)env_n_obs(st) : nullptr);
            else {
                env_rows<Env, NC>(st, eng.pol, perm, ids, rowoff, bad, bad_id);
                if constexpr (EARLY_IDS) {
                    if (writer) {
                        const int n = env_n_obs(st);
                        uint16_t *o = a.obs16 + (e_local * (uint64_t)a.out.t_pad + (uint64_t)t) * (uint64_t)n;
#pragma unroll
                        for (int i = 0; i < NO; ++i) if (i < n) o[i] = (uint16_t)ids[i];
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i) rowoff[i] = -1;
        }
        float lg[4]; float value, rew; int action;
        if constexpr (A > 4) {
            // the masked logits go to their own array (the record's four slots stay zero); a record that is not pushed stores none
            const float *head = eng.forward_head(rowoff, value);
            const uint32_t mb = alive ? st.masks() : 0u;
            rew = alive ? st.reward() : 0.0f;
            float *row = alive && !bad ? a.lgw + (e_local * (uint64_t)a.out.t_pad + (uint64_t)t) * (uint64_t)A : nullptr;
            action = env_gumbel_stream<A>(eng.pol, head, j, eng.g, perm, mb, a.seed, e_global, (uint32_t)t, row);
#pragma unroll
            for (int i = 0; i < 4; ++i) lg[i] = 0.0f;
        } else {
        eng.forward(rowoff, lg, value);
        env_act_perm<A>(eng.pol, perm, lg);
        const uint32_t mb = alive ? st.masks() : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) lg[i] = (i < A && ((mb >> i) & 1u)) ? lg[i] : -1e10f;    // policy.rs:62
        rew = alive ? st.reward() : 0.0f;
        const u32x4 gw = rng_draw(a.seed, e_global, (uint32_t)t, STREAM_GUMBEL);
        action = gumbel_argmax_n<A>(lg, gw);
        }
        if (alive) {
            bool failed = false;
            if (bad) {                                                                // (the host path fails the collect here)
                if (writer) {                                                         // the library names the first one (t, episode)
                    const uint32_t zero4[4] = {0u, 0u, 0u, 0u};
                    store_rec(a.out.rec + e_local * (uint64_t)a.out.t_pad + (uint64_t)t, zero4, lg, __builtin_bit_cast(float, bad_id), bad_count ? 1.0f : 0.0f, 0, -1);
                    atomicOr(a.err, bad_count ? 8u : 1u);
                }
                failed = true;
                alive = false;
            } else {
                if (writer) {                                                         // push the record (ppo.rs:71-76)
                    const uint64_t rec = e_local * (uint64_t)a.out.t_pad + (uint64_t)t;
                    const uint32_t zero4[4] = {0u, 0u, 0u, 0u};
                    store_rec(a.out.rec + rec, zero4, lg, value, rew, action, perm);
                    if constexpr (!EnvHasObserveN<Env>::value && !EARLY_IDS) {        // (observe_n: env_rows_n has stored them)
                        const int n = env_n_obs(st);
                        uint16_t *o = a.obs16 + rec * (uint64_t)n;
#pragma unroll
                        for (int i = 0; i < NO; ++i) if (i < n) o[i] = (uint16_t)ids[i];
                    }
                }
                if (st.is_final()) alive = false;                                     // ppo.rs:78
                else if (t + 1 >= a.out.t_pad) {                                      // the host path's max_records_per_episode
                    if (writer) atomicOr(a.err, 2u);
                    alive = false;
                } else { st.step(action); ++t; }                                      // ppo.rs:79
            }
            // the episode is over: its length at once (the column may go on with another one)
            if (!alive && writer) a.out.ep_len[e_local] = ((uint32_t)t + 1u) | (failed ? 0x80000000u : 0u);
        }
        if (a.queue) {                                                                // (uniform: the barrier depends on it alone)
            const bool want = !alive && more;
            unsigned got = 0xffffffffu;
            if (want && writer) got = atomicAdd(a.queue, 1u);
            unsigned *bc = reinterpret_cast<unsigned *>(eng.lds_user);
            if (writer) bc[j] = got;
            __syncthreads();
            got = bc[j];
            if (want) {
                if ((uint64_t)got < a.num_episodes) {
                    e_taken = got;
                    t = 0; alive = true; fresh = true;                                // (reset at the top of the next step)
                } else more = false;
            }
        }
    }
    eng.end();
