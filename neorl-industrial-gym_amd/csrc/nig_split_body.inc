// nig_split_body.inc -- the body of the three-wave rollout kernels (nig_split.hpp: split_rollout_kernel, split_sampled_kernel).
// Included inside a __global__ function whose argument is `const RolloutArgs q`, with Env, OUT, NP, NOISE and SAMPLED in scope.
    constexpr int S = Env::S, A = Env::A, KS = Env::KS;
    // step noise, if any, in ChemicalReactor's shape (two normals per step from one Philox block per two steps); an env
    // without step noise (RobotAssembly, KS = 0) leaves the producer the action load + clip only
    static_assert(Env::COOP_RESET && !Env::CUSTOM_STEP && S % 4 == 0 && (KS == 0 || (Env::SHARED_STEP_BLOCK && KS == 2)),
                  "three-wave form: cooperative reset, S a multiple of 4, no step noise or ChemicalReactor's");
    constexpr int KN = KS > 0 ? KS : 1;
    using Lds = SplitLds<Env, NP>;
    constexpr int K = Lds::K;
    constexpr int THREADS = 192 * NP;
    // The ring slot of a step is a COMPILE-TIME constant in all three roles: every step loop is unrolled over the K slots
    // (split_unrolled), so slot * HI_SLOT / slot * IH_SLOT ride in the DS instructions' offset fields on one per-lane base
    // address per ring -- no slot counter, compare, select, multiply or address add per step.  (Largest offset: the last
    // slot's last row, below K * IH_SLOT * 4 bytes; the field holds 16 bits.)
    static_assert(K * Lds::IH_SLOT * 4 < 65536 && K * Lds::HI_SLOT * 4 < 65536, "slot offsets must fit the DS offset field");
    __shared__ __attribute__((aligned(16))) unsigned char smem[Lds::BYTES];
    float4 *const s_probit = reinterpret_cast<float4 *>(smem + Lds::OFF_PROBIT);
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    // readfirstlane: the wave index (and everything derived from it: role, ring addresses, row pointers) lives in
    // scalar registers -- the role branches are scalar branches and the row pointers advance on the scalar unit
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned pair = wave % NP, role = wave / NP;          // 0 integrator, 1 producer, 2 recorder
    lds_u32_t *const sync = (lds_u32_t *)(smem + Lds::OFF_SYNC) + pair * 4;
    float *const s_hi = reinterpret_cast<float *>(smem + Lds::OFF_HI) + pair * (K * Lds::HI_SLOT);
    float *const s_ih = reinterpret_cast<float *>(smem + Lds::OFF_IH) + pair * (K * Lds::IH_SLOT);
    for (int i_ = (int)tid; i_ < 768; i_ += THREADS) s_probit[i_] = NIG_PROBIT[i_];
    if (tid < NP * 4) reinterpret_cast<uint32_t *>(smem + Lds::OFF_SYNC)[tid] = 0u;
    __syncthreads();

    const StepArgs &p = q.s;
    const uint32_t base = (blockIdx.x + q.block0) * (64u * NP) + pair * 64u;     // the triple's first lane
    const uint32_t t_base = launch_counter(p.t_ptr, p.t_off) + (uint32_t)q.it0;      // local step i uses t_base + i + 1
    const int n = q.n_steps - q.it0;                                             // local steps [0, n)

    if (role == 0) {
        // ------------------------------------------------------------------ integrator
        float *const s_img = reinterpret_cast<float *>(smem + Lds::OFF_IMG) + pair * (Env::RESET_ROWS * 64);
        unsigned char *const s_wlist = smem + Lds::OFF_WLIST + pair * 64;
        int step = (int)((p.ctr + base)[lane] & NIG_CTR_STEP_MASK);     // the recorder keeps (and stores) the whole counter word
        float s[S], nx[S];
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = (p.state + base + k * p.ld_state)[lane];
        // Inputs are read one step AHEAD: the ring counter and (speculatively) the slot of step i + 1 are read
        // while step i is integrated; the counter is looked at afterwards, and only if the producer had not got
        // that far (it normally is several steps ahead) the wave spins and reads the slot again.  A read issued after
        // the counter read sees at least what the counter promised (DS operations of a wave execute in order).
        // Two input register sets and K ring slots, the loop unrolled by lcm(2, K): no copies between the sets, no slot arithmetic.
        float in0[KS + A], in1[KS + A];
        const float *const hi_l = s_hi + lane;                               // per-lane bases: the slot is an immediate offset on them
        v4f *const ih_row = reinterpret_cast<v4f *>(s_ih) + lane * (S / 4);
        uint32_t *const ih_vb = reinterpret_cast<uint32_t *>(s_ih + S * 64) + lane;
        auto read_inputs = [&](auto sl_tag, float (&dst)[KS + A]) __attribute__((always_inline)) {
            constexpr int sl = decltype(sl_tag)::value;
#pragma unroll
            for (int k = 0; k < KS + A; ++k) dst[k] = hi_l[sl * Lds::HI_SLOT + k * 64];
        };
        // local step i: ring slot i mod K and input register set i mod 2, both static (r = i mod UI)
        constexpr int UI = split_lcm(2, K);
        auto integrate = [&](auto r_tag, const int i) __attribute__((always_inline)) {
            constexpr int r = decltype(r_tag)::value, slot = r % K;
            constexpr std::integral_constant<int, (slot + 1) % K> nslot{};
            const float (&in)[KS + A] = (r & 1) ? in1 : in0;
            float (&in_next)[KS + A] = (r & 1) ? in0 : in1;
            const uint32_t c_next = split_peek(sync + 0);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            read_inputs(nslot, in_next);
            double nz[KN];
            float a[A];
            nz[0] = 0.0;
#pragma unroll
            for (int k = 0; k < KS; ++k) nz[k] = (double)in[k];
#pragma unroll
            for (int k = 0; k < A; ++k) a[k] = in[KS + k];
            const uint32_t vb = Env::violated(s, a) & p.cmask;
            Env::dynamics(s, a, nz, p.dt32, p.dt, nx);
            StepResult<Env> res;
            post_core<Env, float>(nx, a, vb, step, p.max_steps, res);          // the reward part is dead here
            const bool done = res.terminated || res.truncated;
#pragma unroll
            for (int k = 0; k < S / 4; ++k) { v4f v = {nx[4 * k], nx[4 * k + 1], nx[4 * k + 2], nx[4 * k + 3]}; ih_row[slot * (Lds::IH_SLOT / 4) + k] = v; }
            ih_vb[slot * Lds::IH_SLOT] = outcome_word(vb, res.terminated, res.truncated);   // the recorder takes the outcome from here (post_record)
            split_post(sync + 1, (uint32_t)i + 1u, lane);
            step = done ? 0 : step + 1;
            if constexpr (NOISE) {
                if (done) {                        // IndustrialEnv.reset on the recorded draws of this step's row set (base.py:133-155)
                    double rn[Env::KR > 0 ? Env::KR : 1];
                    const double *rnr = p.reset_noise + (size_t)(q.it0 + i) * q.nz_reset_stride + base;
#pragma unroll
                    for (int k = 0; k < Env::KR; ++k) rn[k] = (rnr + (size_t)k * p.ld_noise)[lane];
                    Env::init(rn, nx);
                }
            } else {
#ifdef NIG_DIAG_SPLIT_NORESTART        // (diagnostic builds only, profiles/split_restart: a finishing lane restarts from the MEANS of its initial
            // state -- no ballot branch, no generator, no LDS trip; ring protocol and stores untouched, results are garbage: the
            // launch-time difference to the production build is the upper bound of everything a cheaper restart can give)
            if (done) {
                double zero[Env::KR > 0 ? Env::KR : 1] = {};
                Env::init(zero, nx);
            }
#else
            const unsigned long long m = __builtin_amdgcn_ballot_w64(done);      // (the mask itself: __ballot takes an int, a 0 / 1 register and a compare back)
            if (m != 0ull)
                coop_reset<Env, quick_reset<Env>::value>(m, done, lane, s_img, s_wlist, p.env0 + (uint64_t)base, t_base + (uint32_t)i + 1u,
                                                         p.seed_lo, p.seed_hi, s_probit, nx);
#endif
            }
#pragma unroll
            for (int k = 0; k < S; ++k) s[k] = nx[k];
            if (i + 1 < n && __builtin_amdgcn_readfirstlane(c_next) < (uint32_t)i + 2u) {   // rare: the producer fell behind
                split_wait(sync + 0, (uint32_t)i + 2u);
                read_inputs(nslot, in_next);
            }
        };
        __builtin_amdgcn_s_waitcnt(0x0F70);       // state loads done: no vmcnt wait is carried into the loop
        __builtin_amdgcn_s_setprio(3);            // the critical path of the three: the SIMD's arbiter serves this wave first
        if (n > 0) { split_wait(sync + 0, 1u); read_inputs(std::integral_constant<int, 0>{}, in0); }
        int i = 0;
        for (; i + UI <= n; i += UI) split_unrolled<UI>([&](auto r_tag) __attribute__((always_inline)) { integrate(r_tag, i + decltype(r_tag)::value); });
        // tail: at most UI - 1 steps, at their compile-time positions
        split_unrolled<UI - 1>([&](auto r_tag) __attribute__((always_inline)) { if (i + decltype(r_tag)::value < n) integrate(r_tag, i + decltype(r_tag)::value); });
        // (the store addresses are rebuilt from a fresh copy of the lane index: a per-lane address kept from the loads at the top
        // would live across the unrolled loop, where RobotAssembly has no register to spare)
        unsigned lane_st = lane;
        asm volatile("" : "+v"(lane_st));
#pragma unroll
        for (int k = 0; k < S; ++k) (p.state + base + k * p.ld_state)[lane_st] = s[k];
        NIG_RING_REPORT(p.ring_err, sync, lane);
        return;
    }

    if (role == 1) {
        // ------------------------------------------------------------------ producer
        const uint64_t gi = p.env0 + (uint64_t)(base + lane);
        [[maybe_unused]] const float *ring = p.actions + base;
#ifndef NIG_SPLIT_LA
#define NIG_SPLIT_LA 4
#endif
        constexpr int LA = NIG_SPLIT_LA;                       // actions are loaded LA steps before they are handed on
        float buf[LA][A];
        uint32_t kept0 = 0u, kept1 = 0u;                       // words 2-3 of the current pair's Philox block
        int aslot = SAMPLED ? 0 : q.it0 % q.ring_len;          // ring slot of the action loaded next
        [[maybe_unused]] const float *act_next = ring + (size_t)aslot * q.slot_stride;
        [[maybe_unused]] auto load_action = [&](float (&ab)[A]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < A; ++k) ab[k] = (act_next + k * p.ld_act)[lane];
            aslot = (aslot + 1 == q.ring_len) ? 0 : aslot + 1;
            act_next = (aslot == 0) ? ring : act_next + q.slot_stride;
        };
        float *const hi_l = s_hi + lane;                       // per-lane base: the slot is an immediate offset on it
        uint32_t freed = 0u;                                   // slots the recorder is known to be done with
        // local step j (u = j mod UP, static: ring slot u mod K, action register set r = u mod LA and position in the pair of
        // launch counters)
        constexpr int UP = split_lcm(LA, K);
        auto produce = [&](auto u_tag, const int j) __attribute__((always_inline)) {
            constexpr int r = decltype(u_tag)::value % LA, pslot = decltype(u_tag)::value % K;
            [[maybe_unused]] float (&ab)[A] = buf[r];
            typename Env::fast_noise_t nz[KN];
            if constexpr (KS > 0 && NOISE) {
                const double *nzr = p.step_noise + (size_t)(q.it0 + j) * q.nz_step_stride + base;
#pragma unroll
                for (int k = 0; k < KS; ++k) nz[k] = (nzr + (size_t)k * p.ld_noise)[lane];
            } else if constexpr (KS > 0) {
                ProbitFetch pf[KN];
                if constexpr ((r & 1) == 0) {     // first step of a pair: the pair's Philox block
                    const u32x4 x = Env::step_block(make_key(gi, t_base + (uint32_t)j + 1u, p.seed_lo, p.seed_hi, s_probit));
                    Env::step_noise_fetch(x.x, x.y, s_probit, pf);
                    kept0 = x.z; kept1 = x.w;
                } else {
                    Env::step_noise_fetch(kept0, kept1, s_probit, pf);
                }
                Env::step_noise_eval(pf, nz);
            }
            float a[A];
            if constexpr (SAMPLED) {
                sample_action<Env>(make_key(gi, t_base + (uint32_t)j + 1u, p.seed_lo, p.seed_hi), a);
            } else {
#pragma unroll
            for (int k = 0; k < A; ++k) a[k] = ab[k];
            }
            clip_action<Env, float>(a);
            if (freed + (uint32_t)K < (uint32_t)j + 1u) freed = split_wait(sync + 2, (uint32_t)(j + 1 - K));   // the slot's previous use
#pragma unroll
            for (int k = 0; k < KS; ++k) hi_l[pslot * Lds::HI_SLOT + k * 64] = (float)nz[k];    // exact: the fast-mode noise IS a float (nig_envs.hpp)
#pragma unroll
            for (int k = 0; k < A; ++k) hi_l[pslot * Lds::HI_SLOT + (KS + k) * 64] = a[k];
            NIG_RING_FAULT_GUARD(p.hflags, j) split_post(sync + 0, (uint32_t)j + 1u, lane);
            if constexpr (!SAMPLED) load_action(ab);     // this register set's next use: local step j + LA
        };
        // the loop is unrolled UP times so that the ring slot, every action register set and the position in the pair of launch
        // counters are compile-time (LA even)
        static_assert(LA % 2 == 0 && LA >= 2 && LA <= 8, "even look-ahead depths up to 8");
        if constexpr (!SAMPLED) {
#pragma unroll
        for (int j = 0; j < LA; ++j) load_action(buf[j]);
        }
        int j = 0;
        for (; j + UP <= n; j += UP) split_unrolled<UP>([&](auto u_tag) __attribute__((always_inline)) { produce(u_tag, j + decltype(u_tag)::value); });
        // tail: at most UP - 1 steps
        split_unrolled<UP - 1>([&](auto u_tag) __attribute__((always_inline)) { if (j + decltype(u_tag)::value < n) produce(u_tag, j + decltype(u_tag)::value); });
        NIG_RING_REPORT(p.ring_err, sync, lane);
        return;
    }

    // ---------------------------------------------------------------------- recorder
    // Everything IndustrialEnv.step does after the dynamics (base.py:176-213), the episode bookkeeping and the outputs.
    uint32_t ctr = (p.ctr + base)[lane];                       // mirrors the integrator's counter word
    const bool tally = p.tally != nullptr;
    using ret_t = std::conditional_t<Env::RET_F32, float, double>;
    ret_t ret = tally ? (ret_t)(p.ep_ret + base)[lane] : (ret_t)0;
    LaneTally lt;
    lt.clear();
    float *rew_row = p.reward ? p.reward + base + (size_t)q.it0 * q.out_stride : nullptr;
    uint32_t *fl_row = p.flags ? p.flags + base + (size_t)q.it0 * q.out_stride : nullptr;
    float *obs_row = nullptr;
    if constexpr (OUT == 3) obs_row = q.obs_out + (size_t)q.it0 * q.obs_step_stride + (size_t)base * S;
    if constexpr (OUT == 2) obs_row = q.obs_out + (size_t)q.it0 * q.obs_step_stride + base;
    const v4f *const ih_row = reinterpret_cast<const v4f *>(s_ih) + lane * (S / 4);     // per-lane bases: the slot is an immediate offset on them
    const v4f *const ih_img = reinterpret_cast<const v4f *>(s_ih) + lane;
    const uint32_t *const ih_vb = reinterpret_cast<const uint32_t *>(s_ih + S * 64) + lane;
    const float *const hi_a = s_hi + KS * 64 + lane;
    __builtin_amdgcn_s_waitcnt(0x0F70);           // counter / return loads done: the loop only ever stores
    uint32_t seen = 0u;
    // local step i: ring slot i mod K, static
    auto record = [&](auto sl_tag, const int i) __attribute__((always_inline)) {
        constexpr int cslot = decltype(sl_tag)::value;
        if (seen < (uint32_t)i + 1u) seen = split_wait(sync + 1, (uint32_t)i + 1u);
        // what the integrator left: post-dynamics state (own row, and the wave's rows in lane-contiguous order),
        // violation bits of the pre-state; and the clipped action the step was handed (its P -> I slot is intact
        // until this wave says so)
        float nx[S], a[A];
#pragma unroll
        for (int k = 0; k < S / 4; ++k) { const v4f v = ih_row[cslot * (Lds::IH_SLOT / 4) + k]; nx[4 * k] = v.x; nx[4 * k + 1] = v.y; nx[4 * k + 2] = v.z; nx[4 * k + 3] = v.w; }
        const uint32_t word = ih_vb[cslot * Lds::IH_SLOT];     // violation bits and the step's outcome (outcome_word)
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = hi_a[cslot * Lds::HI_SLOT + k * 64];
        v4f tr[S / 4];
        if constexpr (OUT == 3) {                  // see rollout_body, OUT == 3
#pragma unroll
            for (int k = 0; k < S / 4; ++k) tr[k] = ih_img[cslot * (Lds::IH_SLOT / 4) + 64 * k];
        }
        split_post(sync + 2, (uint32_t)i + 1u, lane);          // (DS order: the reads above execute before this write)
        const int step = (int)(ctr & NIG_CTR_STEP_MASK) + 1;
#ifdef NIG_DIAG_SPLIT_REC_NOCOMPUTE    // (diagnostic builds only, profiles/r05: the recorder as a pure store wave -- no reward, penalties, flags or
        // tally arithmetic, the same LDS reads and the same stores -- the upper bound of what a fourth, store-only wave per triple
        // could give the headline, VERDICT r04 next #7; results are garbage)
        StepRecord<Env> res;
        res.reward = nx[0] + a[0]; res.flags = word; res.nviol = (int)(word & 1u); res.ncrit = 0; res.done = false;
#else
        // the integrator decided how the step ended; reward, penalties and the flag word are this wave's
        const StepRecord<Env> res = post_record<Env>(nx, a, word, step);
#endif
        const uint32_t viol_ep = episode_violations(ctr, res.nviol);
        const bool done = res.done;
        const uint32_t fl = res.flags;
        ctr = counter_word(step, viol_ep);
        if (tally) ret = add_reward<Env>(ret, res.reward);
        if constexpr (OUT == 3) {
            v4f *oo = reinterpret_cast<v4f *>(obs_row);
#pragma unroll
#ifdef NIG_DIAG_SPLIT_PLAINSTORE       // (diagnostic builds only: ordinary instead of streaming stores for the trajectory rows)
            for (int k = 0; k < S / 4; ++k) oo[lane + 64u * k] = tr[k];
#else
            for (int k = 0; k < S / 4; ++k) stream_store(oo + lane + 64u * k, tr[k]);
#endif
        }
        if constexpr (OUT == 2) {
#pragma unroll
            for (int k = 0; k < S; ++k) stream_store(obs_row + k * q.ld_obs_out + lane, nx[k]);
        }
        if constexpr (OUT >= 1) {
            stream_store(rew_row + lane, (float)res.reward);
            stream_store(fl_row + lane, fl);
            rew_row += q.out_stride; fl_row += q.out_stride;
        }
        if constexpr (OUT >= 2) obs_row += q.obs_step_stride;
        if (done) {
            ret = lt.finish(tally, ret, step, viol_ep, res.ncrit);
            ctr = 0u;
        }
    };
    int i = 0;
    for (; i + K <= n; i += K) split_unrolled<K>([&](auto sl_tag) __attribute__((always_inline)) { record(sl_tag, i + decltype(sl_tag)::value); });
    // tail: at most K - 1 steps
    split_unrolled<K - 1>([&](auto sl_tag) __attribute__((always_inline)) { if (i + decltype(sl_tag)::value < n) record(sl_tag, i + decltype(sl_tag)::value); });
    (p.ctr + base)[lane] = ctr;
    if (lt.life != 0) (p.life_viol + base)[lane] += lt.life;
    if (tally) {
        (p.ep_ret + base)[lane] = (double)ret;
        if (lt.episodes > 0) lt.merge(p.tally + base + lane, p.ld, p.n_en);
    }
    NIG_RING_REPORT(p.ring_err, sync, lane);
