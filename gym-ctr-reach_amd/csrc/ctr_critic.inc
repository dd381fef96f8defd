// ctr_critic.inc -- the MLP critic (ctr_critic) and the sampler that hands the learner the DDPG
// target with the batch (ctr_her_sample_td), with their extern "C" entry points.  Included at the
// end of ctr_kernels.hip: the critic is the actor's code (ctr_actor.inc: one layout, one packer, one
// column-tile function) on a 25- or 26-float row with a one-row output layer, and the fused sampler
// is k_her_sample's row (ctr_her_device.inc: her_sample_row) followed by the two networks.
//
// Restates the target-Q part of stable-baselines DDPG (ddpg.py _setup_target_network_updates /
// _train_step): target = r + gamma (1 - done) Q'(s', pi'(s')) from the target networks, whose
// parameters stay with the learner; the blobs are their bf16 view (ctr_actor_load, ctr_critic_load).
// ctr_her_sample_td3 is the same sampler with TD3's target (Fujimoto et al. 2018: target policy
// smoothing and the smaller of two target critics); the reference has no counterpart.
namespace {

__global__ __launch_bounds__(BLOCK) void k_critic(ActorK ck, const float *__restrict__ rows,
                                                  const float *__restrict__ actions, int64_t n, float *__restrict__ q)
{
    char *lds = actor_lds_base(0);
    actor_stage(ck, lds);
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t ee = e < n ? e : n - 1;                 // lanes past n: the clamped row, no write
    const bool multi = ck.in_dim == 26;
    const float *rp = rows + ee * (ck.in_dim - 6), *ap = actions + 6 * ee;
    float row[20], a[6], x[26];
    #pragma unroll
    for (int k = 0; k < 19; ++k) row[k] = rp[k];
    row[19] = multi ? rp[19] : 0.f;
    #pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = ap[i];
    critic_row(row, a, multi, x);
    __syncthreads();
    const float v = critic_wave(ck, lds, x);
    if (e < n) q[e] = v;
}

// Kernel-argument copy of ctr_her_td_t.
struct TdK {
    float gamma;
    float *target, *q_next, *next_action;
};

// r + gamma (1 - done) q as two f32 roundings: numpy's float32 gamma * q + r, bit for bit.
__device__ __forceinline__ float td_target(float rew, float dn, float gamma, float q)
{
#pragma clang fp contract(off)
    const float gq = gamma * q;
    return dn != 0.f ? rew : gq + rew;
}

// k_her_sample, then for the row of each lane: the target policy on the next_obs row the lane just
// staged, the target critic on [next_obs row, a'], the target.  The blobs take turns in one dynamic
// LDS region behind the static row staging: stage the actor, barrier, run it, barrier, stage the
// critic over it, barrier, run it.  Everything around the MFMA code is wave-uniform: the lanes past
// B formed zero rows and compute on them, and only the stores are guarded.
//
// td_next_action: the sampler's row, the flush of the batch and a' = tanhf(the actor's logits) on
// the lane's next_obs row (row[20], as critic_row takes it).  The actor's blob is still in use by
// other waves when it returns: a barrier comes before the region is staged again.
//
// td_next_row is its first half, which ctr_sac.inc's k_her_sample_sac shares: the sampler's row, the
// policy's blob staged beside it, the flush of the batch and the lane's next_obs row in registers.
__device__ __forceinline__ void td_next_row(const ctr_her_t &h, int64_t B, uint64_t seed, uint64_t counter,
                                            const ctr_her_batch_t &out, const ActorK &ak, char *lds, float *s_obs,
                                            float *s_nobs, float *s_act, float &rew, float &dn, float row[20])
{
    her_sample_row(h, B, seed, counter, out, s_obs, s_nobs, s_act, rew, dn);
    actor_stage(ak, lds);
    __syncthreads();                                      // the rows and the actor's blob
    her_flush_batch(h, B, out, s_obs, s_nobs, s_act);
    const bool multi = h.obs_dim == 14;
    const float *sn = s_nobs + threadIdx.x * (h.obs_dim + 6);     // the f32 row as stored to out.next_obs
    #pragma unroll
    for (int k = 0; k < 19; ++k) row[k] = sn[k];
    row[19] = multi ? sn[19] : 0.f;
}

__device__ __forceinline__ void td_next_action(const ctr_her_t &h, int64_t B, uint64_t seed, uint64_t counter,
                                               const ctr_her_batch_t &out, const ActorK &ak, char *lds, float *s_obs,
                                               float *s_nobs, float *s_act, float &rew, float &dn, float row[20],
                                               float a[6])
{
    td_next_row(h, B, seed, counter, out, ak, lds, s_obs, s_nobs, s_act, rew, dn, row);
    float y[6];
    actor_logits(ak, lds, row, y);
    #pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = tanhf(y[i]);
}

// The critic ck on [row, a] from the region every wave is through with: stage, barrier, run.
__device__ __forceinline__ float td_critic(const ActorK &ck, char *lds, const float row[20], const float a[6], bool multi)
{
    float x[26];
    actor_stage(ck, lds);
    __syncthreads();
    critic_row(row, a, multi, x);
    return critic_wave(ck, lds, x);
}

__global__ __launch_bounds__(BLOCK) void k_her_sample_td(HerK hk, int64_t B, uint64_t seed, uint64_t counter,
                                                         ctr_her_batch_t out, ActorK ak, ActorK ck, TdK td)
{
    __shared__ __attribute__((aligned(16))) float s_obs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_nobs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_act[BLOCK * 6];
    const ctr_her_t &h = hk.h;
    float rew, dn, row[20], a[6];
    char *lds = actor_lds_base(0);
    td_next_action(h, B, seed, counter, out, ak, lds, s_obs, s_nobs, s_act, rew, dn, row, a);
    __syncthreads();                                      // every wave is through with the actor's blob
    const float qn = td_critic(ck, lds, row, a, h.obs_dim == 14);
    const float tg = td_target(rew, dn, td.gamma, qn);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < B) {
        td.target[i] = tg;
        if (td.q_next) td.q_next[i] = qn;
        if (td.next_action)
            #pragma unroll
            for (int k = 0; k < 6; ++k) td.next_action[6 * i + k] = a[k];
    }
}

// Kernel-argument copy of ctr_her_td3_t.
struct Td3K {
    float gamma, sigma, clip;
    float *target, *q1_next, *q2_next, *next_action;
};

// TD3's target policy smoothing on row i of the draw (include/ctr_reach_amd.h, "TD3": the
// specification): a += clip(sigma z), clipped to [-1, 1], z from two Philox blocks of stream 7, a
// pure function of (seed, counter, i).  The uniforms and the Box-Muller products are explore_lane's
// (ctr_device.hpp), spelled out in the same way.  sigma == 0: nothing is drawn and the bits stay.
__device__ __forceinline__ void td3_smooth(uint64_t seed, uint64_t counter, uint32_t i, float sigma, float clip, float a[6])
{
#pragma clang fp contract(off)
    if (sigma == 0.f) return;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t c1 = (uint32_t)counter, c3 = (uint32_t)(counter >> 32) ^ (7u << 24);
    uint32_t w0[4] = {0u, c1, i, c3}, w1[4] = {1u, c1, i, c3};
    philox(w0, k0, k1);
    philox(w1, k0, k1);
    const float u[6] = {(float)(w0[0] >> 8) * 0x1p-24f, (float)(w0[1] >> 8) * 0x1p-24f, (float)(w0[2] >> 8) * 0x1p-24f,
                        (float)(w0[3] >> 8) * 0x1p-24f, (float)(w1[0] >> 8) * 0x1p-24f, (float)(w1[1] >> 8) * 0x1p-24f};
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float r = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, u[2 * j]))));
        float sn, cs;
        sincosf(__fmul_rn(6.2831855f, u[2 * j + 1]), &sn, &cs);
        const float z[2] = {__fmul_rn(r, cs), __fmul_rn(r, sn)};
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float e = fminf(fmaxf(__fmul_rn(sigma, z[h]), -clip), clip);
            a[2 * j + h] = fminf(fmaxf(__fadd_rn(a[2 * j + h], e), -1.f), 1.f);
        }
    }
}

// k_her_sample_td with TD3's clipped double-Q target: the smoothed target action, then the two
// target critics, one after the other in the same LDS region, and the smaller q in the target.
__global__ __launch_bounds__(BLOCK) void k_her_sample_td3(HerK hk, int64_t B, uint64_t seed, uint64_t counter,
                                                          ctr_her_batch_t out, ActorK ak, ActorK ck1, ActorK ck2, Td3K td)
{
    __shared__ __attribute__((aligned(16))) float s_obs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_nobs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_act[BLOCK * 6];
    const ctr_her_t &h = hk.h;
    float rew, dn, row[20], a[6];
    char *lds = actor_lds_base(0);
    td_next_action(h, B, seed, counter, out, ak, lds, s_obs, s_nobs, s_act, rew, dn, row, a);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    td3_smooth(seed, counter, (uint32_t)i, td.sigma, td.clip, a);
    const bool multi = h.obs_dim == 14;
    __syncthreads();                                      // every wave is through with the actor's blob
    const float q1 = td_critic(ck1, lds, row, a, multi);
    __syncthreads();                                      // ... and with the first critic's
    const float q2 = td_critic(ck2, lds, row, a, multi);
    const float tg = td_target(rew, dn, td.gamma, fminf(q1, q2));
    if (i < B) {
        td.target[i] = tg;
        if (td.q1_next) td.q1_next[i] = q1;
        if (td.q2_next) td.q2_next[i] = q2;
        if (td.next_action)
            #pragma unroll
            for (int k = 0; k < 6; ++k) td.next_action[6 * i + k] = a[k];
    }
}

// ctr_her_sample's checks (with `fn` in the messages); *tiles = the scan's grid.
int her_sample_check(const char *fn, const ctr_her_t *her, int64_t batch_size, const ctr_her_batch_t *out, int64_t *tiles)
{
    char who[64];
    snprintf(who, sizeof who, "%s: her is NULL", fn);
    if (int r = check_her(her, who)) return r;
    const char *why = nullptr;
    if (!out || batch_size < 0 || batch_size > 0x7fffffff) why = "bad batch";
    else if (batch_size == 0) return 0;
    else if (her->n == 0) why = "empty store";
    else if (!out->obs || !out->action || !out->reward || !out->next_obs || !out->done) why = "output missing";
    else if ((reinterpret_cast<uintptr_t>(out->obs) | reinterpret_cast<uintptr_t>(out->next_obs) |
              reinterpret_cast<uintptr_t>(out->action)) & 15)
        why = "obs / next_obs / action must be 16-byte aligned";
    else {
        const int64_t E = her->n * her->slots;
        *tiles = (E + HER_TILE - 1) / HER_TILE;
        if (*tiles > 0x7fffffff) why = "store too large";
    }
    if (!why) return 0;
    snprintf(g_err, sizeof g_err, "%s: %s", fn, why);
    return CTR_EINVAL;
}

// r != 0: g_err gets `fn` in front unless it starts with it (the store's, the layout and the blob
// checks name only what they looked at).
int td_named(const char *fn, int r)
{
    if (r && strncmp(g_err, fn, strlen(fn)) != 0) {
        char why[sizeof g_err];
        snprintf(why, sizeof why, "%s", g_err);
        snprintf(g_err, sizeof g_err, "%s: %.400s", fn, why);
    }
    return r;
}

}  // namespace

extern "C" {

int64_t ctr_critic_blob_bytes(const ctr_critic_t *c)
{
    ActorK ck;
    if (critic_layout(c, &ck)) return -1;
    return (int64_t)ck.bytes;
}

int ctr_critic_pack(const ctr_critic_t *c, const float *const *W, const float *const *b, void *blob_host)
{
    ActorK ck;
    if (int r = critic_layout(c, &ck)) return r;
    return mlp_pack(ck, "ctr_critic_pack", W, b, blob_host);
}

int ctr_critic_load(const ctr_critic_t *c, const float *const *W, const float *const *b, void *stream)
{
    ActorK ck;
    if (int r = critic_layout(c, &ck)) return r;
    return mlp_load(ck, "critic", "ctr_critic_load", c->blob, W, b, stream);
}

int ctr_critic(const ctr_critic_t *c, const float *rows, const float *actions, int64_t n, float *q, void *stream)
{
    ActorK ck;
    if (int r = critic_check(c, &ck)) return r;
    if (n < 0 || n > 0x7fffffff) return fail(CTR_EINVAL, "ctr_critic: n out of range");
    if (n > 0 && (!rows || !actions || !q)) return fail(CTR_EINVAL, "ctr_critic: rows, actions or q is NULL");
    if (n == 0) return 0;
    const size_t shm = ck.bytes + ACTOR_LDS_SLACK;
    if (int r = allow_dynamic_lds(k_critic, shm)) return r;
    hipLaunchKernelGGL(k_critic, dim3(grid_for(n)), dim3(BLOCK), shm, (hipStream_t)stream, ck, rows, actions, n, q);
    return hip_check("ctr_critic launch");
}

int ctr_her_sample_td(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                      const ctr_her_batch_t *out, const ctr_her_td_t *td, void *stream)
{
    int64_t tiles = 0;
    if (int r = her_sample_check("ctr_her_sample_td", her, batch_size, out, &tiles)) return r;
    if (!td) return fail(CTR_EINVAL, "ctr_her_sample_td: td is NULL");
    ActorK ak, ck;
    if (int r = actor_layout(td->actor, &ak)) return r;          // (not actor_check: the scale is not read)
    if (int r = mlp_blob("actor", td->actor->blob, &ak)) return r;
    if (int r = critic_check(td->critic, &ck)) return r;
    if (ak.in_dim != her->obs_dim + 6)
        return fail(CTR_EINVAL, "ctr_her_sample_td: actor->in_dim must be her->obs_dim + 6");
    if (ck.in_dim != her->obs_dim + 12)
        return fail(CTR_EINVAL, "ctr_her_sample_td: critic->in_dim must be her->obs_dim + 12");
    if (!isfinite(td->gamma)) return fail(CTR_EINVAL, "ctr_her_sample_td: gamma must be finite");
    if (!td->target) return fail(CTR_EINVAL, "ctr_her_sample_td: td->target is NULL");
    if (batch_size == 0) return 0;
    // the row staging is the kernel's static LDS; the larger blob is the dynamic region
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every actor and every critic fit beside the row staging");
    const size_t shm = std::max(ak.bytes, ck.bytes) + ACTOR_LDS_SLACK;
    if (int r = allow_dynamic_lds(k_her_sample_td, shm)) return r;
    const TdK tk = {td->gamma, td->target, td->q_next, td->next_action};
    her_scan(her, tiles, stream);
    hipLaunchKernelGGL(k_her_sample_td, dim3(grid_for(batch_size)), dim3(BLOCK), shm, (hipStream_t)stream, HerK{*her},
                       batch_size, seed, counter, *out, ak, ck, tk);
    return hip_check("ctr_her_sample_td launch");
}

int ctr_her_sample_td3(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                       const ctr_her_batch_t *out, const ctr_her_td3_t *td, void *stream)
{
    const char *fn = "ctr_her_sample_td3";
    int64_t tiles = 0;
    if (int r = td_named(fn, her_sample_check(fn, her, batch_size, out, &tiles))) return r;
    if (!td) return fail(CTR_EINVAL, "ctr_her_sample_td3: td is NULL");
    ActorK ak, ck1, ck2;
    if (int r = td_named(fn, actor_layout(td->actor, &ak))) return r;      // (not actor_check: the scale is not read)
    if (int r = td_named(fn, mlp_blob("actor", td->actor->blob, &ak))) return r;
    if (!td->critic1 || !td->critic2) return fail(CTR_EINVAL, "ctr_her_sample_td3: critic1 or critic2 is NULL");
    if (int r = td_named(fn, critic_check(td->critic1, &ck1))) return r;
    if (int r = td_named(fn, critic_check(td->critic2, &ck2))) return r;
    if (ak.in_dim != her->obs_dim + 6)
        return fail(CTR_EINVAL, "ctr_her_sample_td3: actor->in_dim must be her->obs_dim + 6");
    if (ck1.in_dim != her->obs_dim + 12 || ck2.in_dim != her->obs_dim + 12)
        return fail(CTR_EINVAL, "ctr_her_sample_td3: critic1->in_dim and critic2->in_dim must be her->obs_dim + 12");
    if (!isfinite(td->gamma)) return fail(CTR_EINVAL, "ctr_her_sample_td3: gamma must be finite");
    if (!isfinite(td->sigma) || td->sigma < 0.f) return fail(CTR_EINVAL, "ctr_her_sample_td3: sigma must be finite and >= 0");
    if (!(td->clip >= 0.f)) return fail(CTR_EINVAL, "ctr_her_sample_td3: clip must be >= 0 (INFINITY: no clip)");
    if (!td->target) return fail(CTR_EINVAL, "ctr_her_sample_td3: td->target is NULL");
    if (batch_size == 0) return 0;
    // the row staging is the kernel's static LDS; the largest of the three blobs is the dynamic region
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every actor and every critic fit beside the row staging");
    const size_t shm = std::max(ak.bytes, std::max(ck1.bytes, ck2.bytes)) + ACTOR_LDS_SLACK;
    if (int r = allow_dynamic_lds(k_her_sample_td3, shm)) return r;
    const Td3K tk = {td->gamma, td->sigma, td->clip, td->target, td->q1_next, td->q2_next, td->next_action};
    her_scan(her, tiles, stream);
    hipLaunchKernelGGL(k_her_sample_td3, dim3(grid_for(batch_size)), dim3(BLOCK), shm, (hipStream_t)stream, HerK{*her},
                       batch_size, seed, counter, *out, ak, ck1, ck2, tk);
    return hip_check("ctr_her_sample_td3 launch");
}

}  // extern "C"
