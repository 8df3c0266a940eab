// nig_rollout_policy_body.inc -- the body of the one-wave closed-loop kernels (nig_rollout_policy.hpp: rollout_policy_kernel,
// rollout_policy_disturbed_kernel, rollout_policy_limited_kernel).  Included inside a __global__ function with `const PolicyArgs &q`
// (the kernel's own by-value argument for rollout_policy_kernel), `const DisturbArgs *dq`, `const LimitArgs *lq`, Env, DIST and
// LIM in scope.
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    // The policy struct is staged in LDS: read from global memory inside the loop, every field was a
    // vector load followed by a full vmcnt(0) (the loop's stores may alias it, so hipcc neither hoists
    // the loads nor uses the scalar cache) -- ~20 serialised L2 round trips per step, 60 % of the step.
    __shared__ nig_policy s_pol;
    __shared__ v4f s_tr[BLOCK / 64][16 * S];       // per-wave transpose of the row-major observation rows
    // envs with a cooperative reset (PowerGrid: ~11 finishing lanes per wave and step) renew them wave by wave as
    // the open-loop rollout does (coop_reset); the in-place form ran the whole reset path in every wave every step
    constexpr bool COOP = Env::COOP_RESET;
    __shared__ float s_img[COOP ? (BLOCK / 64) * Env::RESET_ROWS * 64 : 1];
    __shared__ unsigned char s_wlist[COOP ? BLOCK : 1];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(q.pol);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&s_pol);
        for (unsigned i = threadIdx.x; i < sizeof(nig_policy) / 4; i += BLOCK) dst[i] = src[i];
    }
    __shared__ float4 s_probit[768];
    for (int i_ = (int)threadIdx.x; i_ < 768; i_ += BLOCK) s_probit[i_] = NIG_PROBIT[i_];
    __syncthreads();                               // (the block barrier also publishes s_pol)
    const nig_policy *pol = &s_pol;
    const StepArgs &p = q.s;
    const unsigned tid = threadIdx.x;
    const uint32_t base = (blockIdx.x + q.block0) * BLOCK;
    const bool in_range = base + tid < p.B;
    if constexpr (COOP) {
        if (base + (tid & ~63u) >= p.B) return;    // a partial wave keeps all 64 lanes: they are the reset's workers
    } else {
        if (!in_range) return;
    }
    const uint32_t t_base = launch_counter(p.t_ptr, p.t_off);
    const uint64_t gi = p.env0 + (uint64_t)(base + tid);
    const bool autoreset = (p.hflags & NIG_F_AUTORESET) != 0;
    const bool tally = p.tally != nullptr;

    uint32_t ctr = in_range ? (p.ctr + base)[tid] : (uint32_t)NIG_CTR_DONE;     // out-of-range lanes idle as frozen
    float s[S], a[A], n[S], integ[A], eprev[A];
    typename Env::fast_noise_t nz[KSN];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = in_range ? (p.state + base + k * p.ld_state)[tid] : 0.0f;
    // PID memory lives in the handle (baseline_agents.py:55-80: integral and previous error are the agent's,
    // never reset): loaded here, stored at the end, so launches chain exactly
    const bool pid_mem = q.pid != nullptr && pol->kind == NIG_POLICY_PID && in_range;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        integ[j] = pid_mem ? (q.pid + base + (size_t)j * p.ld)[tid] : 0.0f;
        eprev[j] = pid_mem ? (q.pid + base + (size_t)(A + j) * p.ld)[tid] : 0.0f;
    }
    double ret = (tally && in_range) ? (p.ep_ret + base)[tid] : 0.0;
    LaneTally lt;
    lt.clear();
    [[maybe_unused]] bool d_obs = false, d_act = false;
    if constexpr (DIST) disturb_switches<S, A>(*dq, d_obs, d_act);

    for (int it = 0; it < q.n_steps; ++it) {
        const uint32_t orow = (uint32_t)it * q.out_stride;
        bool need_reset = false;
        const bool live = !(ctr & NIG_CTR_DONE);
        if (!live) {                               // frozen lane: base.py:159-160
            if (in_range) {
                if (p.flags) (p.flags + base + orow)[tid] = frozen_flag_word(ctr);
                if (p.reward) (p.reward + base + orow)[tid] = 0.0f;
                if constexpr (LIM) {
                    if (lq->xflags) (lq->xflags + base + orow)[tid] = 0u;
                }
            }
        } else {
        const RngKey key = make_key(gi, t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit);
        if constexpr (DIST) {                      // include/nig.h "nig-disturb-v1": the policy sees o, the plant receives a
            // (the observation draws before the law, the action draws behind it: neither set is live across policy_action)
            float zo[S], za[A], o[S];
            disturb_draws<S, A>(*dq, d_obs, false, gi, key.t, ctr & NIG_CTR_STEP_MASK, p.seed_lo, p.seed_hi, s_probit, zo, za);
            disturb_obs<S>(*dq, d_obs, s, zo, o);
            if (dq->seen_out) disturb_store_seen<S>(*dq, it, (size_t)(base + tid), o);
            policy_action<Env>(pol, o, key, integ, eprev, a);
            disturb_draws<S, A>(*dq, false, d_act, gi, key.t, ctr & NIG_CTR_STEP_MASK, p.seed_lo, p.seed_hi, s_probit, zo, za);
            disturb_act<A>(*dq, d_act, za, a);
        } else {
            policy_action<Env>(pol, s, key, integ, eprev, a);
        }
        if (q.obs_out) {
            // Row-major observations.  When every lane of the wave is live (exists, not frozen) the 64 rows
            // leave through the wave-private LDS image as whole-line streaming stores, as in rollout_kernel;
            // a wave with frozen lanes (their rows stay untouched) or the partial last wave writes row by row.
            // (Only for batches that put several waves on a SIMD: at one wave per SIMD the kernel is
            // issue-bound and the extra LDS round trip costs 5 %, above that it is worth +22 %.)
            if (p.B > 2u * 65536u && __ballot(true) == ~0ull) {
                const unsigned lane = tid & 63u;
                v4f *tr = s_tr[tid >> 6];
                if constexpr (S % 4 == 0) {
#pragma unroll
                    for (int k = 0; k < S / 4; ++k) { v4f v = {s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]}; tr[lane * (S / 4) + k] = v; }
                } else {
                    float *trf = reinterpret_cast<float *>(tr) + lane * S;
#pragma unroll
                    for (int k = 0; k < S; ++k) trf[k] = s[k];
                }
                v4f *oo = reinterpret_cast<v4f *>(q.obs_out + (size_t)it * q.obs_step_stride + (size_t)(base + (tid & ~63u)) * S);
                image_rows_fence();                // other lanes' writes are read below
                constexpr int NV = (16 * S + 63) / 64;
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (16 * S % 64 == 0 || lane + 64u * k < 16u * S) stream_store(oo + lane + 64u * k, tr[lane + 64u * k]);
            } else {
                float *oo = q.obs_out + (size_t)it * q.obs_step_stride + (size_t)(base + tid) * S;
                if constexpr (S % 4 == 0) {
#pragma unroll
                    for (int k = 0; k < S / 4; ++k) store16(oo + 4 * k, s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
                } else {                           // rows that are not a multiple of 16 bytes: dword stores
#pragma unroll
                    for (int k = 0; k < S; ++k) oo[k] = s[k];
                }
            }
        }
        if (q.act_out) {
            float *ao = q.act_out + (size_t)it * q.act_step_stride + base;
#pragma unroll
            for (int j = 0; j < A; ++j) stream_store(ao + j * q.ld_act_out + tid, a[j]);
        }
        if constexpr (KS > 0) Env::draw_step(key, nz); else nz[0] = 0;
        const int step_pre = (int)(ctr & NIG_CTR_STEP_MASK);
        StepResult<Env> res;
        if constexpr (LIM) {                       // the added constraints beside the built-ins (nig_limits.hpp): res counts both kinds
            const uint32_t xf = step_core_limited<Env>((limit_table_ptr)lq->table, s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
            if (lq->xflags) stream_store(lq->xflags + base + orow + tid, xf);
        } else {
            step_core<Env>(s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
        }
        const int step = step_pre + 1;
        const uint32_t viol_ep = episode_violations(ctr, res.nviol);
        const bool done = res.terminated || res.truncated;
        uint32_t fl = pack_flags<Env>(res, step) | did_reset_flag(done && autoreset);
        if constexpr (LIM) fl = limited_flag_counts<Env>(fl, res.viol_bits, res.shutdown);
        ctr = counter_word(step, viol_ep);
        if (tally) ret = add_reward<Env>(ret, res.reward);
        if (p.reward) stream_store(p.reward + base + orow + tid, (float)res.reward);
        if (p.flags) stream_store(p.flags + base + orow + tid, fl);
        if (done) {
            ret = lt.finish(tally, ret, step, viol_ep, res.ncrit);
            if (autoreset) {
                if constexpr (COOP) {
                    need_reset = true;
                } else {
                    double rn[KR > 0 ? KR : 1];
                    Env::draw_init(key, rn);
                    Env::init(rn, n);
                }
                ctr = 0u;
            } else {
                ctr |= NIG_CTR_DONE;
            }
        }
        }   // live
        if constexpr (COOP) {                      // every lane of the wave arrives here, whatever its own state
            const unsigned long long m = __ballot(need_reset);
            if (m != 0ull)
                coop_reset<Env>(m, need_reset, tid & 63u, s_img + (tid >> 6) * (Env::RESET_ROWS * 64), s_wlist + (tid >> 6) * 64,
                                p.env0 + (uint64_t)(base + (tid & ~63u)), t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi,
                                s_probit, n);
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < S; ++k) s[k] = n[k];
        }
    }
    if (!in_range) return;
#pragma unroll
    for (int k = 0; k < S; ++k) (p.state + base + k * p.ld_state)[tid] = s[k];
    store_episode(p.ctr, p.life_viol, p.ep_ret, p.tally, p.ld, p.n_en, base, tid, tally, ctr, lt.life, ret, lt);
    if (pid_mem) {
#pragma unroll
        for (int j = 0; j < A; ++j) {
            (q.pid + base + (size_t)j * p.ld)[tid] = integ[j];
            (q.pid + base + (size_t)(A + j) * p.ld)[tid] = eprev[j];
        }
    }
