// tw_env_solve_loop.hpp -- the step loop of the device-environment evaluate / solve: the BODY of solve_env_kernel and of
// solve_env16_kernel (tw_rollout_env.hpp) and of solve_env16x2_kernel (tw_solve_env16x2.hpp), which include this file inside their
// function bodies.  NO once-pragma and no include guard: it is included three times, once per kernel.  It is no header of its own --
// nothing else may include it.
//
// The including kernel has in scope, before the #include:
//   Env, NC    its template parameters
//   Eng        the engine: EngineV<NC>, EngineV16<NC> or EngineV16x2<NC>
//   a          an EnvSolveArgs, by value or by const reference
//   proto      the prototype, a const Env
//   lds        the dynamic LDS (extern __shared__ float lds[], aligned to 16)
//   eng        a declared `Eng eng`; EngineV16: with eng.img already set; EngineV16x2: with eng.img and eng.err (= a.err, where
//              eng.end() raises GEN16X2_ERR_RANGE) already set
//
// Shared as TEXT and not as a function template, for the reason tw_env_rollout_loop.hpp gives.
    constexpr int A = Env::NUM_ACTIONS, NO = Env::N_OBS;
    eng.begin1(a.pol, lds);
    const int j = eng.j;
    const uint64_t att_first = (uint64_t)blockIdx.x * Eng::EPB + (uint64_t)j;
    const bool valid = att_first < a.num_attempts, writer = eng.h == 0 && eng.primary();
    uint32_t att_taken = 0xffffffffu;                                                 // the attempt taken from the queue; none: att_first
    Env st = proto;
    bool  alive = valid;                                                              // (a fresh attempt: until its reset below says otherwise)
    bool  fresh = valid;                                                              // the column's attempt is still to be reset
    bool  more  = valid && a.queue != nullptr;
    float total = 0.0f;
    int   t = 0;
    eng.begin2();
    while (__syncthreads_or(alive ? 1 : 0)) {
        const uint64_t att = att_taken != 0xffffffffu ? (uint64_t)att_taken : (uint64_t)blockIdx.x * Eng::EPB + (uint64_t)j;
        const uint64_t key = a.episode_offset * (uint64_t)a.num_searches + att;       // keys this attempt's draws
        bool ended = false;                                                           // the attempt ended by itself in this step
        // the ONE place reset() is called from (see tw_env_rollout_loop.hpp).  A fresh attempt whose reset state is already final is over
        // at once (solve.rs:29): its column feeds no row to this step's forward and takes the next attempt at the end of it
        if (fresh) {
            st = proto;                                                               // evaluate.rs:39 / solve.rs:85
            if (!a.from_state) st.reset(a.seed, a.episode_offset + att / a.num_searches);   // the episode keys the start state
            total = 0.0f; t = 0; fresh = false;
            alive = !st.is_final();
            ended = !alive;
        }
        int perm = -1;
        if (eng.pol.n_perms > 0) {
            const u32x4 w = rng_draw(a.seed, key, (uint32_t)t, STREAM_PERM);
            perm = (int)u32_below(w.x, (uint32_t)eng.pol.n_perms);
        }
        int ids[NO], rowoff[NC];
        bool bad = false; int bad_id = 0;
        [[maybe_unused]] bool bad_count = false;
        if (alive) {
            if constexpr (EnvHasObserveN<Env>::value) (void)env_rows_n<Env, NC>(st, eng.pol, perm, ids, rowoff, bad, bad_id, bad_count, nullptr);
            else env_rows<Env, NC>(st, eng.pol, perm, ids, rowoff, bad, bad_id);
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i) rowoff[i] = -1;
        }
        float lg[4], value;
        [[maybe_unused]] const float *head = nullptr;
        if constexpr (A > 4) head = eng.forward_head(rowoff, value);
        else {
            eng.forward(rowoff, lg, value);
            env_act_perm<A>(eng.pol, perm, lg);
        }
        const uint32_t mb = (alive ? st.masks() : 0u) & ((1u << A) - 1u);
        [[maybe_unused]] float probs[4];
        if constexpr (A <= 4) masked_softmax4(lg, mb, probs);                         // policy.rs:43-47 (masked entries add +0.0)
        if (alive) {
            if (bad) {
                if (writer) {
                    atomicOr(a.err, bad_count ? 8u : 1u);
                    a.success[att] = bad_count ? 2.0f : (st.success() ? 1.0f : 0.0f);
                    a.total[att]   = __builtin_bit_cast(float, bad_id);
                    a.n_steps[att] = (uint32_t)t | 0x80000000u;
                }
                alive = false;
            } else {
                total = total + st.reward();                                          // solve.rs:31
                int action = 0;
                if constexpr (A > 4) {
                    float u = 0.0f;
                    if (!a.deterministic) u = u32_to_unit(rng_draw(a.seed, key, (uint32_t)t, STREAM_SOLVE).x);
                    action = env_predict_stream<A>(eng.pol, head, j, perm, mb, a.deterministic != 0u, u);
                } else if (a.deterministic) {
                    float bv = probs[0];
#pragma unroll
                    for (int i = 1; i < A; ++i) if (probs[i] > bv) { bv = probs[i]; action = i; }
                } else {
                    const u32x4 w = rng_draw(a.seed, key, (uint32_t)t, STREAM_SOLVE);
                    action = sample_weighted4(probs, A, u32_to_unit(w.x));
                }
                st.step(action);                                                      // solve.rs:56
                // solve.rs:57-59: the move, into the attempt's own row (alive: att < num_attempts)
                if (writer && a.actions != nullptr && (uint32_t)t < a.actions_stride) a.actions[att * (uint64_t)a.actions_stride + (uint64_t)t] = (uint8_t)action;
                ++t;
                if (st.is_final()) alive = false;
                else if ((uint32_t)t >= a.max_steps) {                                // the host path's max_steps
                    if (writer) atomicOr(a.err, 4u);
                    alive = false;
                }
                ended = !alive;
            }
        }
        if (ended && writer) {                                                        // its results (solve.rs:65-68), after t moves
            a.success[att] = st.success() ? 1.0f : 0.0f;
            a.total[att]   = total + st.reward();
            a.n_steps[att] = (uint32_t)t;
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
                if ((uint64_t)got < a.num_attempts) {
                    att_taken = got;
                    alive = true; fresh = true;                                       // (reset at the top of the next step)
                } else more = false;
            }
        }
    }
    eng.end();
