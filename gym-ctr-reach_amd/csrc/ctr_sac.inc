// ctr_sac.inc -- SAC's three device pieces (include/ctr_reach_amd.h, "SAC": the specification), with
// their extern "C" entry points.  Included at the end of ctr_kernels.hip, after ctr_ddpg.inc.
//
// ctr_gauss_act: the tanh-Gaussian policy.  ctr_actor's MLP (actor_tile, the bf16 blob) with a 12-row
// output layer, rows 0..5 the mean and rows 6..11 the log standard deviation; one row per lane, one
// launch.  The head's device functions (gauss_layout, gauss_logits, gauss_eps, gauss_head) are in
// ctr_gauss.inc, ahead of the period kernels, which run them too (k_collect_gauss).
//
// ctr_sac_actor_step: the policy's update.  k_sac_grad is k_ddpg_grad<true> with three network
// images in LDS instead of two (the policy, critic 1, critic 2), the stochastic head between the
// policy and the critics, and the minimum of the two critics in the loss; the layers, the tiles, the
// slots and their order are ctr_ddpg.inc's device functions.  k_sac_apply is ddpg_apply_element
// (k_ddpg_apply's body) plus one thread that makes the temperature's step.
//
// ctr_her_sample_sac: the replay draw with SAC's soft target.  k_her_sample_sac is k_her_sample_td3
// (ctr_critic.inc: td_next_row, td_critic, td_target) with gauss_logits, gauss_eps and gauss_head
// in the target policy's place.
//
// ctr_collect_gauss: the entry point of k_collect_gauss (ctr_kernels.hip), ctr_collect with the policy's
// sample in the actor's and the noise's place.
namespace {

struct GaussK {
    uint64_t seed, counter, row_base;
    int32_t deterministic;
    float *actions, *unit, *logp, *logits;
};

__global__ __launch_bounds__(BLOCK) void k_gauss_act(ActorK ak, const float *__restrict__ rows, int64_t n, GaussK g)
{
    char *lds = actor_lds_base(0);
    actor_stage(ak, lds);
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const float *row = rows + (e < n ? e : n - 1) * ak.in_dim;     // lanes past n: the clamped row, no write
    float x[20];
    #pragma unroll
    for (int k = 0; k < 19; ++k) x[k] = row[k];
    x[19] = ak.in_dim == 20 ? row[19] : 0.f;
    __syncthreads();
    float y[12], eps[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, t[6];
    gauss_logits(ak, lds, x, y);
    if (!g.deterministic) gauss_eps(g.seed, g.counter, (uint32_t)(g.row_base + (uint64_t)e), eps);
    const float lp = gauss_head(y, eps, g.deterministic != 0, t);
    if (e >= n) return;
    if (g.actions)
        #pragma unroll
        for (int i = 0; i < 6; ++i) g.actions[6 * e + i] = __fmul_rn(ak.scale[i], t[i]);
    if (g.unit)
        #pragma unroll
        for (int i = 0; i < 6; ++i) g.unit[6 * e + i] = t[i];
    if (g.logp) g.logp[e] = lp;
    if (g.logits)
        #pragma unroll
        for (int i = 0; i < 12; ++i) g.logits[12 * e + i] = y[i];
}

// ------------------------------------------------------------------------------------------
// The soft target inside the sampler.  Kernel-argument copy of ctr_her_sac_t.
struct HerSacK {
    float gamma;
    const float *log_alpha;
    float *target, *q1_next, *q2_next, *next_action, *next_logp;
};

// min(q1, q2) - alpha logp as two f32 roundings: numpy's float32 np.minimum(q1, q2) - alpha * logp, bit for bit.
__device__ __forceinline__ float sac_soft_q(float q1, float q2, float alpha, float lp)
{
#pragma clang fp contract(off)
    const float al = alpha * lp;
    return fminf(q1, q2) - al;
}

// k_her_sample_td3 (ctr_critic.inc) with SAC's target: the CURRENT policy's stochastic head on the
// next_obs row the lane just staged, drawn under the sampler's own (seed, counter) -- k_gauss_act's
// draw for row_base 0 --, then the two target critics, one after the other in the same LDS region,
// and the smaller q less alpha logp in the target.  Wave-uniform around the MFMA code, as there:
// the lanes past B compute on their zero rows, and only the stores are guarded.
__global__ __launch_bounds__(BLOCK) void k_her_sample_sac(HerK hk, int64_t B, uint64_t seed, uint64_t counter,
                                                          ctr_her_batch_t out, ActorK ak, ActorK ck1, ActorK ck2, HerSacK td)
{
    __shared__ __attribute__((aligned(16))) float s_obs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_nobs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_act[BLOCK * 6];
    const ctr_her_t &h = hk.h;
    float rew, dn, row[20];
    char *lds = actor_lds_base(0);
    td_next_row(h, B, seed, counter, out, ak, lds, s_obs, s_nobs, s_act, rew, dn, row);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    float y[12], eps[6], t[6];
    gauss_logits(ak, lds, row, y);
    gauss_eps(seed, counter, (uint32_t)i, eps);
    const float lp = gauss_head(y, eps, false, t);
    const bool multi = h.obs_dim == 14;
    __syncthreads();                                      // every wave is through with the policy's blob
    const float q1 = td_critic(ck1, lds, row, t, multi);
    __syncthreads();                                      // ... and with the first critic's
    const float q2 = td_critic(ck2, lds, row, t, multi);
    const float alpha = (float)exp((double)*td.log_alpha);          // a uniform load; f64 so that the host can restate it
    const float soft = sac_soft_q(q1, q2, alpha, lp);
    const float tg = td_target(rew, dn, td.gamma, soft);
    if (i < B) {
        td.target[i] = tg;
        if (td.q1_next) td.q1_next[i] = q1;
        if (td.q2_next) td.q2_next[i] = q2;
        if (td.next_logp) td.next_logp[i] = lp;
        if (td.next_action)
            #pragma unroll
            for (int k = 0; k < 6; ++k) td.next_action[6 * i + k] = t[k];
    }
}

// ------------------------------------------------------------------------------------------
// The policy's step.
constexpr int SAC_HEAD = DDPG_T * 6;              // the (row, action dimension) pairs of a tile
constexpr size_t SAC_LP_BYTES = DDPG_SLOTS * sizeof(double);   // the slots' logp sums, behind the DDPG region

struct SacGradK {
    DdpgNetK net;                      // the policy (out_rows = 12)
    DdpgNetK c1, c2;                   // the critics, read only
    const float *rows;
    const float *log_alpha;
    int32_t B;
    float dq;                          // -1/B: dL/dq of a row on the critic that gave the minimum
    double inv_B;
    float beta1, beta2;
    const float *pow;
    char *ws;
    double *lp_part;
    uint64_t seed, counter;
};

// What the head keeps of a tile between forward and backward, per (row, dimension), and the rows'
// loss and logp terms.  The head runs in f64 on the f32 logits and noise and is rounded to f32 once
// where it meets the f32 networks (the action, dZ), as k_ddpg_grad<true> rounds its tanh.
struct SacTile {
    double term[SAC_HEAD];             // logp's term of the pair
    double es[SAC_HEAD];               // exp(s)
    double t[SAC_HEAD];                // tanh(u)
    double loss[DDPG_T], lp[DDPG_T];
    float eps[SAC_HEAD];
    int32_t open[SAC_HEAD];            // the clip of s is not active
};

__global__ __launch_bounds__(BLOCK) void k_sac_grad(SacGradK k)
{
    __shared__ SacTile s;
    float *lds = reinterpret_cast<float *>(actor_lds_base(0));
    DdpgLds La = {}, L1 = {}, L2 = {};
    lds = ddpg_lds_net(k.net, lds, La);
    lds = ddpg_lds_net(k.c1, lds, L1);
    ddpg_lds_net(k.c2, lds, L2);
    const int row_dim = k.net.in_dim;
    constexpr int SX = DDPG_X0 + DDPG_PAD, SO = DDPG_OUTC + DDPG_PAD;
    float *hdr = reinterpret_cast<float *>(k.ws);
    float *slot = reinterpret_cast<float *>(k.ws + DDPG_HDR) +
                  (size_t)blockIdx.x * ddpg_slot_floats(k.net.params, k.net.biases);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the powers this step's Adam divides by: the apply launch reads these and stores them to pow
        hdr[0] = k.pow[0] * k.beta1;
        hdr[1] = k.pow[1] * k.beta2;
    }
    const double alpha = exp((double)*k.log_alpha);        // the value from before this step's update
    const double aB = alpha * k.inv_B;
    const int ntiles = (k.B + DDPG_T - 1) / DDPG_T;
    double lsum = 0.0, lpsum = 0.0;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x, first = false) {
        const int r0 = tile * DDPG_T;
        // the tile's input rows, zero past B and past in_dim (the critics' action columns come from the head)
        for (int i = (int)threadIdx.x; i < DDPG_T * DDPG_X0; i += BLOCK) {
            const int r = i / DDPG_X0, c = i - r * DDPG_X0;
            const float x = r0 + r < k.B && c < row_dim ? k.rows[(size_t)(r0 + r) * row_dim + c] : 0.f;
            La.x0[r * SX + c] = x;
            L1.x0[r * SX + c] = x;
            L2.x0[r * SX + c] = x;
        }
        if (threadIdx.x < DDPG_T) {
            const int r = (int)threadIdx.x;
            float z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (r0 + r < k.B) gauss_eps(k.seed, k.counter, (uint32_t)(r0 + r), z);
            #pragma unroll
            for (int j = 0; j < 6; ++j) s.eps[6 * r + j] = z[j];
        }
        __syncthreads();
        ddpg_forward(k.net, La);
        if (threadIdx.x < SAC_HEAD) {
            const int i = (int)threadIdx.x, r = i / 6, j = i - 6 * r;
            const float ys = La.out[r * SO + 6 + j];
            const double mu = (double)La.out[r * SO + j], eps = (double)s.eps[i];
            const double sd = fmin(fmax((double)ys, -20.0), 2.0);
            const double es = exp(sd), u = mu + es * eps, t = tanh(u);
            const double x = -2.0 * u, sp = fmax(x, 0.0) + log1p(exp(-fabs(x)));
            s.term[i] = (-0.5 * eps * eps - sd - 0.91893853320467274178) - 2.0 * (0.69314718055994530942 - u - sp);
            s.es[i] = es;
            s.t[i] = t;
            s.open[i] = ys >= -20.f && ys <= 2.f;
            const float a = (float)t;
            L1.x0[r * SX + row_dim + j] = a;
            L2.x0[r * SX + row_dim + j] = a;
        }
        __syncthreads();
        ddpg_forward(k.c1, L1);
        ddpg_forward(k.c2, L2);
        if (threadIdx.x < DDPG_T) {
            const int r = (int)threadIdx.x;
            const bool valid = r0 + r < k.B;
            float *q1 = L1.out + r * SO, *q2 = L2.out + r * SO;
            const bool second = *q2 < *q1;                 // a tie: critic 1
            double lp = 0.0;
            #pragma unroll
            for (int j = 0; j < 6; ++j) lp += s.term[6 * r + j];
            s.lp[r] = valid ? lp : 0.0;
            s.loss[r] = valid ? alpha * lp - (double)(second ? *q2 : *q1) : 0.0;
            *q1 = valid && !second ? k.dq : 0.f;
            *q2 = valid && second ? k.dq : 0.f;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            #pragma unroll
            for (int r = 0; r < DDPG_T; ++r) {
                lsum += s.loss[r];
                lpsum += s.lp[r];
            }
        ddpg_backward(k.c1, L1, false, nullptr, first, row_dim >> 4);
        ddpg_backward(k.c2, L2, false, nullptr, first, row_dim >> 4);
        if (threadIdx.x < SAC_HEAD) {
            const int i = (int)threadIdx.x, r = i / 6, j = i - 6 * r;
            const bool valid = r0 + r < k.B;
            // dL/dt from both critics (one of them is zero), through tanh; logp's own d/du = 2 t, d/ds = -1
            const double dt = (double)L1.x0[r * SX + row_dim + j] + (double)L2.x0[r * SX + row_dim + j];
            const double t = s.t[i];
            const double du = dt * (1.0 - t * t) + aB * (2.0 * t);
            const double ds = du * (s.es[i] * (double)s.eps[i]) - aB;
            La.out[r * SO + j] = valid ? (float)du : 0.f;
            La.out[r * SO + 6 + j] = valid && s.open[i] ? (float)ds : 0.f;
        }
        __syncthreads();
        ddpg_backward(k.net, La, true, slot, first, 0);
    }
    if (threadIdx.x == 0) {
        reinterpret_cast<double *>(k.ws + 16)[blockIdx.x] = lsum;
        k.lp_part[blockIdx.x] = lpsum;
    }
}

// The temperature's part of the apply launch.
struct SacAlphaK {
    float *log_alpha, *state, *grad, *logp_mean;
    const double *lp_part;
    int32_t slots, learn;
    double inv_B;
    float target_entropy, lr, beta1, beta2, eps;
};

// k_ddpg_apply's work on the policy; the grid's last thread sums the slots' logp, stores the mean and
// the temperature's gradient -(logp_mean + target_entropy), and with learn makes log_alpha's Adam step.
__global__ __launch_bounds__(BLOCK) void k_sac_apply(DdpgApplyK k, SacAlphaK a)
{
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == BLOCK - 1) {
        double sum = a.lp_part[0];
        for (int i = 1; i < a.slots; ++i) sum += a.lp_part[i];
        const float mean = (float)(sum * a.inv_B);
        const float g = -__fadd_rn(mean, a.target_entropy);
        if (a.logp_mean) *a.logp_mean = mean;
        if (a.grad) *a.grad = g;
        if (a.learn) {
            float m = a.state[0], v = a.state[1];
            const float pw1 = a.state[2] * a.beta1, pw2 = a.state[3] * a.beta2;
            *a.log_alpha = ddpg_adam(*a.log_alpha, g, m, v, a.lr, a.beta1, a.beta2, a.eps, pw1, pw2);
            a.state[0] = m;
            a.state[1] = v;
            a.state[2] = pw1;
            a.state[3] = pw2;
        }
    }
    ddpg_apply_element(k);
}

constexpr size_t SAC_STATIC_LDS = sizeof(SacTile);

// The shapes of a SAC learner's three networks (the policy with its 12-row head).
int sac_shapes(const char *fn, const ctr_actor_t *actor, const ctr_critic_t *c1, const ctr_critic_t *c2,
                      DdpgNetK *an, DdpgNetK *n1, DdpgNetK *n2)
{
    ActorK ak;
    if (!actor) return ddpg_fail(fn, "actor is NULL");
    if (!c1 || !c2) return ddpg_fail(fn, "critic1 or critic2 is NULL");
    if (int r = td_named(fn, gauss_layout(actor, &ak))) return r;
    ddpg_shape(ak, an);
    if (int r = td_named(fn, critic_layout(c1, &ak))) return r;
    ddpg_shape(ak, n1);
    if (int r = td_named(fn, critic_layout(c2, &ak))) return r;
    ddpg_shape(ak, n2);
    if (an->in_dim + 6 != n1->in_dim || an->in_dim + 6 != n2->in_dim)
        return ddpg_fail(fn, "actor->in_dim + 6 must be critic->in_dim of both critics");
    return 0;
}

}  // namespace

extern "C" {

int64_t ctr_gauss_blob_bytes(const ctr_actor_t *a)
{
    ActorK ak;
    if (gauss_layout(a, &ak)) return -1;
    return (int64_t)ak.bytes;
}

int ctr_gauss_pack(const ctr_actor_t *a, const float *const *W, const float *const *b, void *blob_host)
{
    ActorK ak;
    if (int r = gauss_layout(a, &ak)) return r;
    return mlp_pack(ak, "ctr_gauss_pack", W, b, blob_host);
}

int ctr_gauss_load(const ctr_actor_t *a, const float *const *W, const float *const *b, void *stream)
{
    ActorK ak;
    if (int r = gauss_layout(a, &ak)) return r;
    return mlp_load(ak, "actor", "ctr_gauss_load", a->blob, W, b, stream);
}

int ctr_gauss_act(const ctr_actor_t *a, const float *rows, int64_t n, uint64_t seed, uint64_t counter, int64_t row_base,
                  int32_t deterministic, float *actions, float *unit, float *logp, float *logits, void *stream)
{
    const char *fn = "ctr_gauss_act";
    ActorK ak;
    if (int r = td_named(fn, gauss_layout(a, &ak))) return r;
    for (int i = 0; i < 6; ++i) {
        if (!isfinite(a->scale[i])) return ddpg_fail(fn, "scale must be finite");
        ak.scale[i] = a->scale[i];
    }
    if (int r = td_named(fn, mlp_blob("actor", a->blob, &ak))) return r;
    if (n < 0 || n > 0x7fffffff) return ddpg_fail(fn, "n out of range");
    if (row_base < 0 || row_base + n > 0x100000000ll) return ddpg_fail(fn, "row_base + n must stay within 0..2^32");
    if (n > 0 && !rows) return ddpg_fail(fn, "rows is NULL");
    if (n == 0) return 0;
    const size_t shm = ak.bytes + ACTOR_LDS_SLACK;
    if (int r = allow_dynamic_lds(k_gauss_act, shm)) return r;
    const GaussK g = {seed, counter, (uint64_t)row_base, deterministic, actions, unit, logp, logits};
    hipLaunchKernelGGL(k_gauss_act, dim3(grid_for(n)), dim3(BLOCK), shm, (hipStream_t)stream, ak, rows, n, g);
    return hip_check("ctr_gauss_act launch");
}

int ctr_her_sample_sac(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                       const ctr_her_batch_t *out, const ctr_her_sac_t *td, void *stream)
{
    const char *fn = "ctr_her_sample_sac";
    int64_t tiles = 0;
    // (batch_size <= 2^31 - 1 here, so the row index fits the noise key's 32-bit word)
    if (int r = td_named(fn, her_sample_check(fn, her, batch_size, out, &tiles))) return r;
    if (!td) return ddpg_fail(fn, "td is NULL");
    ActorK ak, ck1, ck2;
    if (int r = td_named(fn, gauss_layout(td->actor, &ak))) return r;          // (the scale is not read)
    if (int r = td_named(fn, mlp_blob("actor", td->actor->blob, &ak))) return r;
    if (!td->critic1 || !td->critic2) return ddpg_fail(fn, "critic1 or critic2 is NULL");
    if (int r = td_named(fn, critic_check(td->critic1, &ck1))) return r;
    if (int r = td_named(fn, critic_check(td->critic2, &ck2))) return r;
    if (ak.in_dim != her->obs_dim + 6) return ddpg_fail(fn, "actor->in_dim must be her->obs_dim + 6");
    if (ck1.in_dim != her->obs_dim + 12 || ck2.in_dim != her->obs_dim + 12)
        return ddpg_fail(fn, "critic1->in_dim and critic2->in_dim must be her->obs_dim + 12");
    if (!isfinite(td->gamma)) return ddpg_fail(fn, "gamma must be finite");
    if (!td->log_alpha) return ddpg_fail(fn, "td->log_alpha is NULL");
    if (!td->target) return ddpg_fail(fn, "td->target is NULL");
    if (batch_size == 0) return 0;
    // the row staging is the kernel's static LDS; the largest of the three blobs is the dynamic region
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every policy and every critic fit beside the row staging");
    const size_t shm = std::max(ak.bytes, std::max(ck1.bytes, ck2.bytes)) + ACTOR_LDS_SLACK;
    if (int r = allow_dynamic_lds(k_her_sample_sac, shm)) return r;
    const HerSacK tk = {td->gamma, td->log_alpha, td->target, td->q1_next, td->q2_next, td->next_action, td->next_logp};
    her_scan(her, tiles, stream);
    hipLaunchKernelGGL(k_her_sample_sac, dim3(grid_for(batch_size)), dim3(BLOCK), shm, (hipStream_t)stream, HerK{*her},
                       batch_size, seed, counter, *out, ak, ck1, ck2, tk);
    return hip_check("ctr_her_sample_sac launch");
}

int ctr_collect_gauss(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_actor_t *policy, uint64_t seed,
                      uint64_t counter, const ctr_her_t *her, int32_t k, const ctr_step_out_t *out, int32_t autoreset,
                      const ctr_rollout_aux_t *aux, void *stream)
{
    const char *fn = "ctr_collect_gauss";
    KCfg kc;
    ActorK ak;
    ctr_rollout_aux_t ax;
    size_t shm = 0;
    // ctr_rollout's checks on the 12-row policy, then ctr_collect's of the store, under this name
    if (int r = td_named(fn, rollout_check(cfg, batch, policy, k, out, autoreset, aux, &kc, &ak, &ax, &shm, true))) return r;
    if (int r = td_named(fn, check_her(her, "ctr_step_her: her is NULL"))) return r;
    if (batch->n != her->n) return ddpg_fail(fn, "batch and store sizes differ");
    if (batch->env_base != her->env_base) return ddpg_fail(fn, "batch and store env_base differ");
    if (her->t_max != cfg->max_steps)
        return ddpg_fail(fn, "her->t_max must equal cfg->max_steps (episodes close at the time limit)");
    // the global env id is the noise key's 32-bit row word, as ctr_gauss_act's row_base + row
    if (batch->env_base < 0 || batch->env_base > 0x100000000ll - batch->n)
        return ddpg_fail(fn, "batch->env_base + n must stay within 0..2^32");
    const ctr_batch_t b = *batch;
    const ctr_step_out_t o = *out;
    if (b.n == 0) return 0;
    const GaussKeyK gk = {seed, counter};
    const HerK hk = {*her};
    CTR_LAUNCH_PERIOD(k_collect_gauss, kc.mode, , dim3(grid_for(b.n)), shm, (hipStream_t)stream, kc, b, ak, k, o,
                      autoreset, ax, gk, hk);
    return hip_check("ctr_collect_gauss launch");
}

int64_t ctr_sac_workspace_bytes(const ctr_actor_t *actor, const ctr_critic_t *critic1, const ctr_critic_t *critic2,
                                int64_t max_B)
{
    const char *fn = "ctr_sac_workspace_bytes";
    DdpgNetK an, c1, c2;
    if (sac_shapes(fn, actor, critic1, critic2, &an, &c1, &c2)) return -1;
    if (max_B < 1 || max_B > DDPG_MAX_B) {
        ddpg_fail(fn, "max_B must be in 1..65536");
        return -1;
    }
    // ctr_td3_critic_step's two regions; or the policy's region with the slots' logp sums behind it
    const int64_t twin = ddpg_ws_bytes(c1.params, c1.biases, max_B) + ddpg_ws_bytes(c2.params, c2.biases, max_B);
    return std::max(twin, ddpg_ws_bytes(an.params, an.biases, max_B) + (int64_t)SAC_LP_BYTES);
}

int ctr_sac_actor_step(const ctr_actor_t *actor, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam,
                       const ctr_critic_t *const critic[2], const float *const *const critic_W[2],
                       const float *const *const critic_b[2], const float *rows, int64_t B, uint64_t seed,
                       uint64_t counter, float *log_alpha, const ctr_sac_alpha_t *alpha_state, float target_entropy,
                       float *loss, float *logp_mean, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "ctr_sac_actor_step";
    SacGradK gk = {};
    DdpgApplyK ap;
    if (!critic || !critic_W || !critic_b) return ddpg_fail(fn, "critic, critic_W or critic_b is NULL");
    if (int r = sac_shapes(fn, actor, critic[0], critic[1], &gk.net, &gk.c1, &gk.c2)) return r;
    if (int r = ddpg_learn_check(fn, net, adam, B, workspace, workspace_bytes, &gk.net, &ap)) return r;
    const int64_t lp_off = ddpg_ws_bytes(gk.net.params, gk.net.biases, B);
    if (workspace_bytes < lp_off + (int64_t)SAC_LP_BYTES) return ddpg_fail(fn, "workspace too small (ctr_sac_workspace_bytes)");
    if (!log_alpha || !alpha_state) return ddpg_fail(fn, "log_alpha or alpha_state is NULL");
    if (!alpha_state->state) return ddpg_fail(fn, "alpha_state->state is NULL");
    if (!isfinite(target_entropy) || !isfinite(alpha_state->lr)) return ddpg_fail(fn, "target_entropy and alpha_state->lr must be finite");
    DdpgNetK *const cn[2] = {&gk.c1, &gk.c2};
    const int nt = 2 * (gk.net.n_hidden + 1);
    // what the step writes besides the policy's tensors, and what it only reads
    const void *const written[6] = {log_alpha, alpha_state->state, alpha_state->grad, loss, logp_mean, ap.pow};
    for (int y = 0; y < 2; ++y) {
        if (!critic_W[y] || !critic_b[y]) return ddpg_fail(fn, "NULL entry in critic_W[2] or critic_b[2]");
        for (int l = 0; l <= cn[y]->n_hidden; ++l) {
            const float *const rd[2] = {critic_W[y][l], critic_b[y][l]};
            if (!rd[0] || !rd[1]) return ddpg_fail(fn, "NULL layer among critic_W, critic_b [0..n_hidden]");
            cn[y]->W[l] = rd[0];
            cn[y]->b[l] = rd[1];
            for (int h = 0; h < 2; ++h) {
                for (int t = 0; t < nt; ++t)
                    if (rd[h] == ap.p[t] || rd[h] == ap.g[t] || rd[h] == ap.m[t] || rd[h] == ap.v[t])
                        return ddpg_fail(fn, "a critic tensor is a tensor of the policy's net (the critics are only read)");
                for (int w = 0; w < 6; ++w)
                    if (rd[h] == written[w]) return ddpg_fail(fn, "a critic tensor is one of the step's outputs");
            }
        }
    }
    for (int w = 0; w < 5; ++w) {
        if (!written[w]) continue;
        for (int t = 0; t < nt; ++t)
            if (written[w] == ap.p[t] || written[w] == ap.g[t] || written[w] == ap.m[t] || written[w] == ap.v[t])
                return ddpg_fail(fn, "log_alpha, its state or an output is a tensor of the policy's net");
        for (int u = w + 1; u < 6; ++u)
            if (written[w] == written[u]) return ddpg_fail(fn, "log_alpha, its state, pow and the outputs must be distinct");
        if (written[w] == rows) return ddpg_fail(fn, "rows is one of the step's outputs");
    }
    const size_t net_bytes[3] = {ddpg_lds_floats(gk.net) * sizeof(float), ddpg_lds_floats(gk.c1) * sizeof(float),
                                 ddpg_lds_floats(gk.c2) * sizeof(float)};
    const size_t shm = net_bytes[0] + net_bytes[1] + net_bytes[2] + ACTOR_LDS_SLACK;
    if (SAC_STATIC_LDS + shm > LDS_PER_WORKGROUP) {
        snprintf(g_err, sizeof g_err, "%s: the tile images of the policy (%zu B), critic 1 (%zu B) and critic 2 (%zu B) + the "
                 "kernel's static LDS (%zu B) exceed the %zu B of LDS of a workgroup", fn, net_bytes[0], net_bytes[1],
                 net_bytes[2], SAC_STATIC_LDS + ACTOR_LDS_SLACK, LDS_PER_WORKGROUP);
        return CTR_EINVAL;
    }
    if (B > 0 && !rows) return ddpg_fail(fn, "rows is NULL");
    if (B == 0) return 0;
    if (int r = allow_dynamic_lds(k_sac_grad, shm)) return r;
    gk.rows = rows;
    gk.log_alpha = log_alpha;
    gk.B = (int32_t)B;
    gk.dq = (float)(-1.0 / (double)B);
    gk.inv_B = 1.0 / (double)B;
    gk.beta1 = ap.beta1;
    gk.beta2 = ap.beta2;
    gk.pow = ap.pow;
    gk.ws = const_cast<char *>(ap.ws);
    gk.lp_part = reinterpret_cast<double *>(gk.ws + lp_off);
    gk.seed = seed;
    gk.counter = counter;
    ap.loss_scale = 1.0 / (double)B;
    ap.loss = loss;
    const SacAlphaK al = {log_alpha, alpha_state->state, alpha_state->grad, logp_mean, gk.lp_part, ap.slots,
                          alpha_state->learn != 0, 1.0 / (double)B, target_entropy, alpha_state->lr, ap.beta1, ap.beta2, ap.eps};
    hipLaunchKernelGGL(k_sac_grad, dim3((unsigned)ap.slots), dim3(BLOCK), shm, (hipStream_t)stream, gk);
    hipLaunchKernelGGL(k_sac_apply, dim3(grid_for(ap.params)), dim3(BLOCK), 0, (hipStream_t)stream, ap, al);
    return hip_check("ctr_sac_actor_step launch");
}

}  // extern "C"
