// tw_env_mcts_loop.hpp -- the search loop of the device-environment self-play and MCTS-guided evaluate: the BODY of mcts_env_kernel
// and of mcts_env16_kernel (tw_mcts_env.hpp), which include this file inside their function bodies.  NO once-pragma and no include
// guard: it is included twice, once per kernel.  It is no header of its own -- nothing else may include it.
//
// The including kernel has in scope, before the #include:
//   Env, NC    its template parameters
//   Eng        the engine: EngineV<NC> or EngineV16<NC> (begin1 / begin2 / forward / forward_head / end, owns_lane, lds_floats, EPB)
//   a          an EnvMctsArgs, by value
//   proto      the prototype, a const Env
//   lds        the dynamic LDS (extern __shared__ float lds[], aligned to 16): the engine's share, then the pending ids of the 16
//              columns (env_mcts_pending_bytes), then with more than four actions their rows of A floats (env_mcts_probs_bytes)
//   eng        a declared `Eng eng`; EngineV16: with eng.img already set
// and at namespace scope what tw_mcts_env.hpp declares above its kernels: EnvNode, EN_NONE, EP_ROOT / EP_LEAF / EP_DONE,
// env_twist_row, env_sample_stream.
//
// Everything behind the heads -- the twist average, the soft-max, expand, the UCB descent, the samples, back-propagation, the visit
// counts, the RNG streams, col_err and the limits -- is this one f32 text in one order for both engines; the engines differ in the
// Linears and the embedding sum alone.  Shared as TEXT and not as a function template, for the reason tw_env_rollout_loop.hpp gives.
    constexpr int A = Env::NUM_ACTIONS, NO = Env::N_OBS;
    constexpr uint32_t AMASK = (1u << A) - 1u;
    constexpr uint32_t ACT_BITS = A > 4 ? 0xffu : 3u;                 // a node's action is a byte of meta (four actions: two bits of it)
    eng.begin1(a.pol, lds);
    const int j = eng.j;
    const uint64_t e_local = (uint64_t)blockIdx.x * Eng::EPB + (uint64_t)j;
    const bool valid = e_local < a.num_columns;
    const bool pub   = eng.h == 0 && eng.owns_lane();                // the lane that publishes column j's ids
    const bool owner = valid && pub;                                  // ... and walks / mutates its tree
    const bool solve = a.solve_on != 0;
    // solve mode: column = ATTEMPT (episode, search); its draws are keyed like single_solve's (solve_env_kernel)
    const uint64_t sv_ep = solve ? a.episode_offset + e_local / a.attempts : 0;
    const uint64_t e_global = solve ? sv_ep * (uint64_t)a.attempts + e_local % a.attempts : a.episode_offset + e_local;
    EnvNode *nodes = reinterpret_cast<EnvNode *>(a.arena) + (valid ? e_local : 0) * (uint64_t)a.node_cap;
    const uint32_t S = a.num_searches, MED = a.max_expand_depth;
    const uint64_t rec_base = e_local * (uint64_t)a.out.t_pad;
    int *pend = reinterpret_cast<int *>(lds + Eng::lds_floats(a.pol)) + j * NO;     // the ids of column j's pending state
    // A > 4: column j's row of A floats behind the ids -- the twist average of the action head, then (owner lane, in place) the
    // probabilities of the pending state, then at the end of a move the visit counts and the move's probabilities
    [[maybe_unused]] float *prow = nullptr;
    if constexpr (A > 4) prow = lds + Eng::lds_floats(a.pol) + GEN_COLS * NO + j * A;

    Env st = proto;                                                   // the episode's env (az.rs:56-57 / evaluate.rs:39)
    if (owner && !a.from_state) st.reset(a.seed, solve ? sv_ep : e_global);       // (from_state: the prototype as it is, solve.rs:85)
    Env cur = st;                                                     // the state of `node`: the one whose evaluation is pending
    int      phase = owner ? EP_ROOT : EP_DONE;
    if (solve && owner && st.is_final()) phase = EP_DONE;             // `while !env.is_final()` (solve.rs:30)
    float    total = 0.0f;                                            // solve mode: summed rewards (solve.rs:25-34)
    uint32_t it = 0, expanded = 0, node = 0, n_nodes = 0, evals = 0;
    int      t = 0;
    float    value = 0.0f;
    uint32_t fail_kind = 0;                                           // 1 + (0: a bad id, 1: a bad count, 2: too long)

    auto end_column = [&](uint32_t kind, uint32_t what, uint32_t bit) {   // (owner) the column stops; the library names the first
        uint32_t *ce = a.col_err + 4 * e_local;
        ce[0] = kind + 1u; ce[1] = evals; ce[2] = what; ce[3] = 0u;
        atomicOr(a.err, bit);
        fail_kind = kind + 1u;
        phase = EP_DONE;
    };
    // the pending state's ids -> the lanes that feed the forward; guarded here: what leaves the owner is an id < obs_size or -1
    auto publish = [&]() {
        if (!pub) return;
        int ids[NO], rows[NC];
        bool bad = false; int bad_id = 0;
        [[maybe_unused]] bool bad_count = false;
        if (phase != EP_DONE) {
            if constexpr (EnvHasObserveN<Env>::value) (void)env_rows_n<Env, NC>(cur, eng.pol, -1, ids, rows, bad, bad_id, bad_count, nullptr);
            else env_rows<Env, NC>(cur, eng.pol, -1, ids, rows, bad, bad_id);
            if (bad) end_column(bad_count ? 1u : 0u, (uint32_t)bad_id, bad_count ? 8u : 1u);
        }
        const bool live = phase != EP_DONE;
#pragma unroll
        for (int i = 0; i < NO; ++i) pend[i] = (live && i < NC) ? rows[i] : -1;
    };
    publish();
    eng.begin2();

    for (;;) {
        if (!__syncthreads_or(phase != EP_DONE ? 1 : 0)) break;       // (the barrier publishes the ids)
        // ---- Policy::full_predict of the pending states (policy.rs:102-126); the engine takes a column's rows from wave 0 ----
        int pid[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) pid[i] = i < NO ? pend[i] : -1;
        float lsum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, vsum = 0.0f;
        const int n_pass = eng.pol.n_perms > 0 ? eng.pol.n_perms : 1;
        const float np = (float)eng.pol.n_perms;
        for (int pass = 0; pass < n_pass; ++pass) {
            const int perm = eng.pol.n_perms > 0 ? pass : -1;
            int rowoff[NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) rowoff[i] = env_twist_row(eng.pol, perm, pid[i]);
            float lg[4], v;
            if constexpr (A > 4) {
                // the head stays in LDS (EngineV::forward_head); lane group g owns the sums of the actions g and g + 16 of its column
                const float *head = eng.forward_head(rowoff, v);
                if (eng.pol.n_perms > 0) vsum = vsum + v / np; else vsum = v;
#pragma unroll 1
                for (int i = eng.g; i < A; i += GEN_COLS) {
                    const float x = head[env_head_unit<A>(eng.pol, perm, i) * GEN_STRIDE + j];
                    if (eng.pol.n_perms > 0) prow[i] = (pass == 0 ? 0.0f : prow[i]) + x / np;    // policy.rs:112-114, from 0.0f in pass order
                    else prow[i] = x;
                }
                __syncthreads();                                                 // (the next forward rewrites the head; the owner reads the sums)
            } else {
            eng.forward(rowoff, lg, v);
            env_act_perm<A>(eng.pol, perm, lg);
            if (eng.pol.n_perms > 0) {
                vsum = vsum + v / np;                                            // policy.rs:111
#pragma unroll
                for (int i = 0; i < 4; ++i) lsum[i] = lsum[i] + lg[i] / np;      // policy.rs:112-114
            } else {
                vsum = v;
#pragma unroll
                for (int i = 0; i < 4; ++i) lsum[i] = lg[i];
            }
            }
        }

        // ---- per-episode tree work on the owner lane -------------------------------------------------------------------------
        if (owner && phase != EP_DONE) {
            float probs[4];
            if constexpr (A > 4) {
                // masked_softmax4 over A values, in place: tw_expf of the allowed sums, added in index order, / (sum + 1e-6f)
                const uint32_t mb = cur.masks() & AMASK;
                float sum = 0.0f;
#pragma unroll 1
                for (int i = 0; i < A; ++i) {
                    const float p = ((mb >> i) & 1u) ? tw_expf(prow[i]) : 0.0f;
                    prow[i] = p;
                    sum = sum + p;
                }
                const float den = sum + 0.000001f;
#pragma unroll 1
                for (int i = 0; i < A; ++i) prow[i] = prow[i] / den;
            } else
            masked_softmax4(lsum, cur.masks() & AMASK, probs);
            const float nn_value = vsum;
            ++evals;
            float pri[4] = {0.0f, 0.0f, 0.0f, 0.0f};                  // priors of the children just created, in child order
            uint32_t acts = 0;                                        // ... and their actions, 2 bits each
            // expand (search.rs:56-75): one child per action with prior > 0
            auto expand = [&](uint32_t idx) -> uint32_t {
                uint32_t cnt = 0;
                acts = 0;
                if constexpr (A > 4) {
#pragma unroll 1
                    for (int act = 0; act < A; ++act) {
                        const float p = prow[act];
                        if (!(p > 0.0f)) continue;
                        EnvNode nn;
                        nn.value_sum = 0.0f; nn.visit = 0; nn.prior = p; nn.parent = idx; nn.child_base = 0;
                        nn.meta = 0u | ((uint32_t)act << 8);
                        nn.pad[0] = 0; nn.pad[1] = 0;
                        nodes[n_nodes + cnt] = nn;
                        ++cnt;
                    }
                } else {
#pragma unroll
                for (int act = 0; act < A; ++act) {
                    if (!(probs[act] > 0.0f)) continue;
                    if (cnt == 0) pri[0] = probs[act]; else if (cnt == 1) pri[1] = probs[act];
                    else if (cnt == 2) pri[2] = probs[act]; else pri[3] = probs[act];
                    acts |= (uint32_t)act << (2 * cnt);
                    EnvNode nn;
                    nn.value_sum = 0.0f; nn.visit = 0; nn.prior = probs[act]; nn.parent = idx; nn.child_base = 0;
                    nn.meta = 0u | ((uint32_t)act << 8);
                    nn.pad[0] = 0; nn.pad[1] = 0;
                    nodes[n_nodes + cnt] = nn;
                    ++cnt;
                }
                }
                nodes[idx].child_base = n_nodes;
                nodes[idx].meta = (nodes[idx].meta & ~0xffu) | cnt;
                n_nodes += cnt;
                return cnt;
            };
            // backpropagate (search.rs:45-53): value_sum += v, visit_count += 1 from the node up to the root
            auto backprop = [&](uint32_t idx, float val) {
                while (idx != EN_NONE) {
                    const EnvNode n = nodes[idx];
                    uint2 w; w.x = __float_as_uint(n.value_sum + val); w.y = n.visit + 1u;
                    *reinterpret_cast<uint2 *>(&nodes[idx].value_sum) = w;
                    idx = n.parent;
                }
            };

            if (phase == EP_ROOT) {
                // root node (search.rs:120-129): visit_count 1, expanded with the root priors
                EnvNode r;
                r.value_sum = 0.0f; r.visit = 1; r.prior = 0.0f; r.parent = EN_NONE; r.child_base = 0;
                r.meta = 0u | (0xffu << 8); r.pad[0] = 0; r.pad[1] = 0;
                nodes[0] = r; n_nodes = 1;
                expand(0u);
                it = 0;
            } else {
                // the leaf just evaluated (search.rs:154-159): expand, sample a child by the priors (next_sample, :94-100); the state follows
                const uint32_t cb = n_nodes;
                const uint32_t nch = expand(node);
                if (nch > 0) {
                    const u32x4 w = rng_draw(a.seed, e_global, it * MED + expanded, STREAM_MCTS | ((uint32_t)t << 8));
                    if constexpr (A > 4) {
                        // the priors are read back from the children just written, in child order
                        const int k = env_sample_stream([&](int c) { return nodes[cb + (uint32_t)c].prior; }, (int)nch, u32_to_unit(w.x));
                        node = cb + (uint32_t)k;
                        cur.step((int)((nodes[node].meta >> 8) & ACT_BITS));
                    } else {
                    const int k = sample_weighted4(pri, (int)nch, u32_to_unit(w.x));
                    node = cb + (uint32_t)k;
                    cur.step((int)((acts >> (2 * k)) & 3u));
                    }
                }
                value = nn_value;
                ++expanded;
            }
            bool resume = (phase == EP_LEAF);
            for (;;) {
                if (!resume) {
                    if (it == S) {
                        // ---- move finished: visit counts -> probs (search.rs:166-188) -----------------------------------------
                        float mp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        const EnvNode root = nodes[0];
                        const uint32_t rnc = root.meta & 0xffu;
                        if constexpr (A > 4) {
                            // the visit counts go into the column's row by action (the probabilities it held are used up: the root
                            // was expanded when they arrived), are summed in index order and divided in place
#pragma unroll 1
                            for (int i = 0; i < A; ++i) prow[i] = 0.0f;
#pragma unroll 1
                            for (uint32_t c = 0; c < rnc; ++c) {
                                const EnvNode ch = nodes[root.child_base + c];
                                const uint32_t act = (ch.meta >> 8) & ACT_BITS;
                                if (act < (uint32_t)A) prow[act] = (float)ch.visit;
                            }
                            float sum = 0.0f;
#pragma unroll 1
                            for (int i = 0; i < A; ++i) sum = sum + prow[i];
                            const bool some = sum > 0.0f;
#pragma unroll 1
                            for (int i = 0; i < A; ++i) prow[i] = some ? prow[i] / sum : 1.0f / (float)A;
                        } else {
                        for (uint32_t c = 0; c < rnc; ++c) {
                            const EnvNode ch = nodes[root.child_base + c];
                            const int act = (int)((ch.meta >> 8) & 3u);
                            const float vis = (float)ch.visit;
                            mp[0] = act == 0 ? vis : mp[0]; mp[1] = act == 1 ? vis : mp[1];
                            mp[2] = act == 2 ? vis : mp[2]; mp[3] = act == 3 ? vis : mp[3];
                        }
                        float sum = 0.0f;
#pragma unroll
                        for (int i = 0; i < A; ++i) sum = sum + mp[i];
                        if (sum > 0.0f) {
#pragma unroll
                            for (int i = 0; i < A; ++i) mp[i] = mp[i] / sum;
                        } else {
#pragma unroll
                            for (int i = 0; i < A; ++i) mp[i] = 1.0f / (float)A;
                        }
                        }
                        if (solve) {
                            // solve.rs:31-58: total += reward; action = argmax | sample of the MCTS probs; step
                            total = total + st.reward();
                            int action = 0;
                            if constexpr (A > 4) {
                                if (a.deterministic) {
                                    float bv = prow[0];
#pragma unroll 1
                                    for (int i = 1; i < A; ++i) { const float p = prow[i]; if (p > bv) { bv = p; action = i; } }
                                } else {
                                    const u32x4 w = rng_draw(a.seed, e_global, (uint32_t)t, STREAM_SOLVE);
                                    action = env_sample_stream([&](int i) { return prow[i]; }, A, u32_to_unit(w.x));
                                }
                            } else
                            if (a.deterministic) {
                                float bv = mp[0];
#pragma unroll
                                for (int i = 1; i < A; ++i) if (mp[i] > bv) { bv = mp[i]; action = i; }
                            } else {
                                const u32x4 w = rng_draw(a.seed, e_global, (uint32_t)t, STREAM_SOLVE);
                                action = sample_weighted4(mp, A, u32_to_unit(w.x));
                            }
                            // solve.rs:56-59: the move, into the column's own row (owner: e_local < num_columns), and the step.  A 32-bit
                            // index: the launcher refuses rows beyond 4 GiB, and EngineV<64> has no register to spare for a wider one
                            if (a.actions != nullptr && (uint32_t)t < a.actions_stride) a.actions[(uint32_t)e_local * a.actions_stride + (uint32_t)t] = (uint8_t)action;
                            st.step(action);
                            ++t;
                            if (st.is_final()) { phase = EP_DONE; break; }
                            if ((uint32_t)t >= a.max_steps) { end_column(2u, 0u, 4u); break; }     // the host path's max_steps
                            phase = EP_ROOT; cur = st;
                            break;
                        }
                        // az.rs:72-81: action = sample(mcts_probs); val = env.reward(); store the record
                        const u32x4 w = rng_draw(a.seed, e_global, (uint32_t)t, STREAM_AZ_ACT);
                        int action;
                        if constexpr (A > 4) action = env_sample_stream([&](int i) { return prow[i]; }, A, u32_to_unit(w.x));
                        else action = sample_weighted4(mp, A, u32_to_unit(w.x));
                        const uint64_t rec = rec_base + (uint64_t)t;
                        const uint32_t zero4[4] = {0u, 0u, 0u, 0u};
                        store_rec(a.out.rec + rec, zero4, mp, 0.0f, st.reward(), 0, -1);      // (A > 4: the four slots are zero)
                        if constexpr (A > 4) {
                            float *row = a.pw + rec * (uint64_t)A;
#pragma unroll 1
                            for (int i = 0; i < A; ++i) row[i] = prow[i];
                        }
                        {
                            // the ids of the state the move's search was rooted in (guarded when it was evaluated)
                            const int stride = env_n_obs(st);
                            uint16_t *o = a.obs16 + rec * (uint64_t)stride;
                            int ids[NO];
                            int n = stride;
                            if constexpr (EnvHasObserveN<Env>::value) { n = st.observe_n(ids); if ((unsigned)n > (unsigned)stride) n = 0; }
                            else st.observe(ids);
#pragma unroll
                            for (int i = 0; i < NO; ++i) if (i < stride) o[i] = i < n ? (uint16_t)ids[i] : (uint16_t)0xFFFFu;
                        }
                        if (st.is_final()) {                                                             // az.rs:84
                            a.out.ep_len[e_local] = (uint32_t)t + 1u;
                            phase = EP_DONE;
                            break;
                        }
                        if (t + 1 >= a.out.t_pad) {                                                      // the host path's max_records_per_episode
                            a.out.ep_len[e_local] = (uint32_t)t + 1u;
                            end_column(2u, 0u, 2u);
                            break;
                        }
                        st.step(action);                                                                 // az.rs:89
                        ++t;
                        phase = EP_ROOT; cur = st;
                        break;
                    }
                    // ---- descend to a leaf by UCB (search.rs:133-138, next :77-91, ucb :29-39); the state follows the actions ----
                    node = 0; cur = st;
                    EnvNode cn = nodes[0];
                    for (;;) {
                        const uint32_t nch = cn.meta & 0xffu, cb = cn.child_base;
                        if (nch == 0) break;
                        uint32_t best = EN_NONE; float best_ucb = -__builtin_inff();
                        EnvNode bestn = cn;
                        const float sq = sqrtf((float)cn.visit);
                        if constexpr (A > 4) {
#pragma unroll 1
                            for (uint32_t c = 0; c < nch; ++c) {          // a rolled loop over the node's own children
                                const EnvNode ch = nodes[cb + c];
                                const float q = ch.visit == 0 ? 0.0f : ch.value_sum / (float)ch.visit;
                                float d = sq / ((float)ch.visit + 1.0f);
                                d = a.C * d;
                                d = d * ch.prior;
                                const float u = q + d;
                                if (u > best_ucb) { best = cb + c; best_ucb = u; bestn = ch; }
                            }
                        } else {
                        EnvNode chs[A];
#pragma unroll
                        for (int c = 0; c < A; ++c) chs[c] = nodes[cb + ((uint32_t)c < nch ? (uint32_t)c : nch - 1u)];
#pragma unroll
                        for (int c = 0; c < A; ++c) {
                            const EnvNode &ch = chs[c];
                            const float q = ch.visit == 0 ? 0.0f : ch.value_sum / (float)ch.visit;
                            float d = sq / ((float)ch.visit + 1.0f);
                            d = a.C * d;
                            d = d * ch.prior;
                            const float u = q + d;
                            if ((uint32_t)c < nch && u > best_ucb) { best = cb + (uint32_t)c; best_ucb = u; bestn = ch; }
                        }
                        }
                        if (best == EN_NONE) break;                   // all-NaN UCB: the reference panics here
                        node = best; cn = bestn;
                        cur.step((int)((bestn.meta >> 8) & ACT_BITS));
                    }
                    value = 0.0f; expanded = 0;
                }
                resume = false;
                // leaf phase (search.rs:143-160)
                bool need_nn = false;
                while (expanded < MED) {
                    value = cur.reward();                                             // :146
                    if (cur.is_final()) break;                                        // :149
                    phase = EP_LEAF; need_nn = true;                                  // :154 needs the network
                    break;
                }
                if (need_nn) break;
                backprop(node, value);                                                // :163
                ++it;
            }
        }
        publish();                                                    // (the ids were read before the forward's first barrier)
    }
    if (owner) {
        if (solve) {
            total = total + st.reward();                                  // solve.rs:65-66
            a.success[e_local] = st.success() ? 1.0f : 0.0f;              // solve.rs:68
            a.total[e_local]   = total;
            a.n_steps[e_local] = (uint32_t)t;
        } else if (fail_kind == 1u || fail_kind == 2u) {
            a.out.ep_len[e_local] = 1u;                                   // (a bad id: the collect fails; the scan still reads a length)
        }
        atomicAdd(a.eval_count, (unsigned long long)evals);
    }
    eng.end();
