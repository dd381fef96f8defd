// ctr_critic.inc -- the MLP critic (ctr_critic) and the sampler that hands the learner the DDPG
// target with the batch (ctr_her_sample_td), with their extern "C" entry points.  Included at the
// end of ctr_kernels.hip: the critic is the actor's code (ctr_actor.inc: one layout, one packer, one
// column-tile function) on a 25- or 26-float row with a one-row output layer, and the fused sampler
// is k_her_sample's row (ctr_her_device.inc: her_sample_row) followed by the two networks.
//
// Restates the target-Q part of stable-baselines DDPG (ddpg.py _setup_target_network_updates /
// _train_step): target = r + gamma (1 - done) Q'(s', pi'(s')) from the target networks, whose
// parameters stay with the learner; the blobs are their bf16 view (ctr_actor_load, ctr_critic_load).
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
// staged, the target critic on [next_obs row, a'], the target.  The two blobs take turns in one
// dynamic LDS region behind the static row staging: stage the actor, barrier, run it, barrier,
// stage the critic over it, barrier, run it.  Everything around the MFMA code is wave-uniform: the
// lanes past B formed zero rows and compute on them, and only the stores are guarded.
__global__ __launch_bounds__(BLOCK) void k_her_sample_td(HerK hk, int64_t B, uint64_t seed, uint64_t counter,
                                                         ctr_her_batch_t out, ActorK ak, ActorK ck, TdK td)
{
    __shared__ __attribute__((aligned(16))) float s_obs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_nobs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_act[BLOCK * 6];
    const ctr_her_t &h = hk.h;
    float rew, dn;
    her_sample_row(h, B, seed, counter, out, s_obs, s_nobs, s_act, rew, dn);
    char *lds = actor_lds_base(0);
    actor_stage(ak, lds);
    __syncthreads();                                      // the rows and the actor's blob
    her_flush_batch(h, B, out, s_obs, s_nobs, s_act);
    const bool multi = h.obs_dim == 14;
    const float *sn = s_nobs + threadIdx.x * (h.obs_dim + 6);     // the f32 row as stored to out.next_obs
    float row[20], y[6], a[6], x[26];
    #pragma unroll
    for (int k = 0; k < 19; ++k) row[k] = sn[k];
    row[19] = multi ? sn[19] : 0.f;
    actor_logits(ak, lds, row, y);
    #pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = tanhf(y[i]);
    __syncthreads();                                      // every wave is through with the actor's blob
    actor_stage(ck, lds);
    __syncthreads();
    critic_row(row, a, multi, x);
    const float qn = critic_wave(ck, lds, x);
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
    hipLaunchKernelGGL(k_her_scan_tiles, dim3((unsigned)tiles), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her});
    hipLaunchKernelGGL(k_her_scan_tops, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her}, tiles);
    hipLaunchKernelGGL(k_her_sample_td, dim3(grid_for(batch_size)), dim3(BLOCK), shm, (hipStream_t)stream, HerK{*her},
                       batch_size, seed, counter, *out, ak, ck, tk);
    return hip_check("ctr_her_sample_td launch");
}

}  // extern "C"
