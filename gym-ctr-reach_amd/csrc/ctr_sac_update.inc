// ctr_sac_update.inc -- a run of SAC updates from one call (ctr_sac_update; include/ctr_reach_amd.h,
// "A run of SAC updates": the specification).  Included at the end of ctr_kernels.hip, after
// ctr_update_common.inc (the tails' arguments and tensor selection, the host checks both update calls share).
//
// An update is what ctr_her_sample_sac, ctr_td3_critic_step, ctr_sac_actor_step, ctr_gauss_load and
// ctr_polyak leave, in five launches instead of nine: the sampler's two scans run once per call (the
// call only reads the store), k_her_sample_sac, k_td3_grad and k_sac_grad are launched as those calls
// launch them, and the two kernels here are the tails behind the gradient launches.
//
// The tails' mapping is k_actor_load's and k_polyak's (ctr_actor.inc: actor_item): one thread per
// 16 B of a blob owns the eight weights or four bias floats that item packs, and the fragment layout
// covers every (row, k) of a layer once, so every parameter has one owner.  For its elements a thread
// does what one thread per parameter did in k_td3_apply / k_sac_apply (the slots' sum in slot order,
// the gradient's store, ddpg_adam), then
//   k_sac_critic_tail: polyak_lerp of the target with the NEW online value, the target's store, and
//                      the target's blob item (k_polyak's work; k_sac_grad reads the online critics
//                      only, so the soft update may run ahead of the policy's step);
//   k_sac_policy_tail: the policy's blob item from the new parameters (k_actor_load's work), and one
//                      thread makes the temperature's step (k_sac_apply's).
// Item 0's thread has element 0's duties (pow, the loss).  The arithmetic per element is the
// functions' the replaced kernels call: ddpg_adam, polyak_lerp, actor_item_pack.
namespace {

// Four consecutive elements of one tensor, from element i on; n of them exist (0..4).  vec: the run
// is whole and is moved as one 16-B access (a hidden layer's weights).
struct SacRun {
    int i, n;
    bool vec;
};

__device__ __forceinline__ void sac_run_load(const float *p, const SacRun &r, float x[4])
{
    if (r.vec) {
        const actor_f32x4u a = *reinterpret_cast<const actor_f32x4u *>(p + r.i);
        #pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = a[j];
    } else {
        #pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = j < r.n ? p[r.i + j] : 0.f;
    }
}

__device__ __forceinline__ void sac_run_store(float *p, const SacRun &r, const float x[4])
{
    if (r.vec) {
        *reinterpret_cast<actor_f32x4u *>(p + r.i) = actor_f32x4u{x[0], x[1], x[2], x[3]};
    } else {
        #pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < r.n) p[r.i + j] = x[j];
    }
}

// ddpg_apply_element's work on the run's elements of tensor `tensor` (ts: its place in a slot and its
// tensors, update_tensors), and the LERP of the target's.  x: the new values the blob item packs (the
// target's with LERP, else the parameters'); past n: +0.
template <bool LERP>
__device__ __forceinline__ void sac_tail_run(const UpdateTailK &k, const SacRun &r, int tensor, const UpdateTensors &ts,
                                             float pw1, float pw2, float x[4])
{
    if (r.n == 0) {
        // a padding item (a row or a bias past the layer's): nothing to sum, +0 in the blob
        #pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = 0.f;
        return;
    }
    const DdpgApplyK &a = k.ap;
    const float *part = reinterpret_cast<const float *>(a.ws + DDPG_HDR);
    const int64_t stride = ddpg_slot_floats(a.params, a.biases);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (tensor & 1) {
        // a bias: the slots' f64 sums, rounded once
        const double *bp = reinterpret_cast<const double *>(part + ddpg_slot_w(a.params)) + ts.bo + r.i;
        #pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < r.n) {
                double s = bp[j];
                for (int t = 1; t < a.slots; ++t) s += bp[(size_t)t * (stride / 2) + j];
                g[j] = (float)s;
            }
    } else {
        const SacRun rs = {ts.first + r.i, r.n, r.vec};
        sac_run_load(part, rs, g);
        for (int t = 1; t < a.slots; ++t) {
            float q[4];
            sac_run_load(part + (size_t)t * stride, rs, q);
            #pragma unroll
            for (int j = 0; j < 4; ++j) g[j] += q[j];
        }
    }
    float pv[4], m[4], v[4], tv[4] = {0.f, 0.f, 0.f, 0.f};
    sac_run_load(ts.p, r, pv);
    sac_run_load(ts.mp, r, m);
    sac_run_load(ts.vp, r, v);
    if (LERP) sac_run_load(ts.tp, r, tv);
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < r.n) {
            pv[j] = ddpg_adam(pv[j], g[j], m[j], v[j], a.lr, a.beta1, a.beta2, a.eps, pw1, pw2);
            if (LERP) tv[j] = polyak_lerp(tv[j], pv[j], k.tau);
        }
        x[j] = j < r.n ? (LERP ? tv[j] : pv[j]) : 0.f;
    }
    sac_run_store(ts.gp, r, g);
    sac_run_store(ts.p, r, pv);
    sac_run_store(ts.mp, r, m);
    sac_run_store(ts.vp, r, v);
    if (LERP) sac_run_store(ts.tp, r, tv);
}

// A tail's work of one thread: item blockIdx.x * BLOCK + threadIdx.x of k's blob.
template <bool LERP>
__device__ __forceinline__ void sac_tail_item(const UpdateTailK &k)
{
    const DdpgApplyK &a = k.ap;
    const float *hdr = reinterpret_cast<const float *>(a.ws);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const float pw1 = hdr[0], pw2 = hdr[1];
    if (i == 0) ddpg_apply_head(a, k.hist, pw1, pw2);
    if (i >= k.ak.bytes / 16) return;
    const ActorItem it = actor_item(k.ak, i);
    const int tensor = 2 * it.l + (it.bias ? 1 : 0);
    const UpdateTensors ts = update_tensors(k, it);
    // the item's elements as two runs of four: actor_item_load's, in the order actor_item_pack takes them
    SacRun r[2] = {{0, 0, false}, {0, 0, false}};
    if (it.bias) {
        r[0].i = it.e;
        r[0].n = min(max(it.rows - it.e, 0), 4);
    } else if (it.row < it.rows) {
        const int base = it.row * it.cols;
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kc = actor_k_of(it.l, it.S, it.h, 4 * h);
            r[h].i = base + kc;
            r[h].n = it.l == 0 ? min(max(it.cols - kc, 0), 4) : 4;
            r[h].vec = it.l != 0;
        }
    }
    float v[8];
    sac_tail_run<LERP>(k, r[0], tensor, ts, pw1, pw2, v);
    sac_tail_run<LERP>(k, r[1], tensor, ts, pw1, pw2, v + 4);
    static_cast<uint4 *>(const_cast<void *>(k.ak.blob))[i] = actor_item_pack(it, v);
}

// The critics' tail: plane blockIdx.y works on critic y and its target (the grid's x is the larger
// blob's; the threads past a blob's items leave).
__global__ __launch_bounds__(BLOCK) void k_sac_critic_tail(UpdateTailK k0, UpdateTailK k1)
{
    if (blockIdx.y == 0) sac_tail_item<true>(k0);
    else sac_tail_item<true>(k1);
}

// The policy's tail; the grid's last thread makes the temperature's step as k_sac_apply's does, and
// writes the history row's logp_mean and log_alpha.
__global__ __launch_bounds__(BLOCK) void k_sac_policy_tail(UpdateTailK k, SacAlphaK a, float *hist)
{
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == BLOCK - 1) {
        double sum = a.lp_part[0];
        for (int i = 1; i < a.slots; ++i) sum += a.lp_part[i];
        const float mean = (float)(sum * a.inv_B);
        const float g = -__fadd_rn(mean, a.target_entropy);
        float la = *a.log_alpha;
        if (a.logp_mean) *a.logp_mean = mean;
        if (a.grad) *a.grad = g;
        if (a.learn) {
            float m = a.state[0], v = a.state[1];
            const float pw1 = a.state[2] * a.beta1, pw2 = a.state[3] * a.beta2;
            la = ddpg_adam(la, g, m, v, a.lr, a.beta1, a.beta2, a.eps, pw1, pw2);
            *a.log_alpha = la;
            a.state[0] = m;
            a.state[1] = v;
            a.state[2] = pw1;
            a.state[3] = pw2;
        }
        if (hist) {
            hist[3] = mean;
            hist[4] = la;
        }
    }
    sac_tail_item<false>(k);
}

}  // namespace

extern "C" {

int ctr_sac_update(const ctr_sac_update_t *u, int32_t updates, void *stream)
{
    const char *fn = "ctr_sac_update";
    if (!u) return ddpg_fail(fn, "u is NULL");
    if (updates < 0) return ddpg_fail(fn, "updates must be >= 0");
    const int64_t B = u->batch_size;
    // ---- ctr_her_sample_sac's checks
    int64_t tiles = 0;
    if (int r = td_named(fn, her_sample_check(fn, u->her, B, u->batch, &tiles))) return r;
    ActorK ak, tk[2];
    if (int r = td_named(fn, gauss_layout(u->policy, &ak))) return r;          // (the scale is not read)
    if (int r = td_named(fn, mlp_blob("actor", u->policy->blob, &ak))) return r;
    if (!u->critic_targ[0] || !u->critic_targ[1]) return ddpg_fail(fn, "critic_targ[0] or critic_targ[1] is NULL");
    for (int y = 0; y < 2; ++y)
        if (int r = td_named(fn, critic_check(u->critic_targ[y], &tk[y]))) return r;
    const ctr_her_t *her = u->her;
    if (ak.in_dim != her->obs_dim + 6) return ddpg_fail(fn, "policy->in_dim must be her->obs_dim + 6");
    if (tk[0].in_dim != her->obs_dim + 12 || tk[1].in_dim != her->obs_dim + 12)
        return ddpg_fail(fn, "critic_targ[0]->in_dim and critic_targ[1]->in_dim must be her->obs_dim + 12");
    if (!isfinite(u->gamma)) return ddpg_fail(fn, "gamma must be finite");
    if (!u->log_alpha) return ddpg_fail(fn, "log_alpha is NULL");
    if (!u->target) return ddpg_fail(fn, "target is NULL");
    // ---- ctr_td3_critic_step's, on the batch's obs, action and the target
    DdpgGradK gk[2] = {};
    DdpgApplyK ap[2];
    const char *null_entry = "NULL entry in critic[2] or critic_net[2]";
    if (!u->critic[0] || !u->critic[1] || !u->critic_net[0] || !u->critic_net[1]) return ddpg_fail(fn, null_entry);
    if (int r = ddpg_critics_check(fn, 2, u->critic, u->critic_net, u->critic_adam, B, u->workspace, u->workspace_bytes,
                                   null_entry, "workspace too small (ctr_sac_workspace_bytes)", gk, ap))
        return r;
    // ---- ctr_sac_actor_step's, on the batch's obs
    SacGradK sk = {};
    DdpgApplyK pp;
    if (int r = sac_shapes(fn, u->policy, u->critic[0], u->critic[1], &sk.net, &sk.c1, &sk.c2)) return r;
    if (int r = ddpg_learn_check(fn, u->policy_net, u->policy_adam, B, u->workspace, u->workspace_bytes, &sk.net, &pp)) return r;
    const int64_t lp_off = ddpg_ws_bytes(sk.net.params, sk.net.biases, B);
    if (u->workspace_bytes < lp_off + (int64_t)SAC_LP_BYTES) return ddpg_fail(fn, "workspace too small (ctr_sac_workspace_bytes)");
    const ctr_sac_alpha_t *al = u->alpha;
    if (!al) return ddpg_fail(fn, "alpha is NULL");
    if (!al->state) return ddpg_fail(fn, "alpha->state is NULL");
    if (!isfinite(u->target_entropy) || !isfinite(al->lr)) return ddpg_fail(fn, "target_entropy and alpha->lr must be finite");
    for (int y = 0; y < 2; ++y) {
        DdpgNetK &cn = y ? sk.c2 : sk.c1;
        for (int l = 0; l <= cn.n_hidden; ++l) {
            cn.W[l] = gk[y].net.W[l];
            cn.b[l] = gk[y].net.b[l];
        }
    }
    const size_t net_bytes[3] = {ddpg_lds_floats(sk.net) * sizeof(float), ddpg_lds_floats(sk.c1) * sizeof(float),
                                 ddpg_lds_floats(sk.c2) * sizeof(float)};
    const size_t shm_sac = net_bytes[0] + net_bytes[1] + net_bytes[2] + ACTOR_LDS_SLACK;
    if (SAC_STATIC_LDS + shm_sac > LDS_PER_WORKGROUP) {
        snprintf(g_err, sizeof g_err, "%s: the tile images of the policy (%zu B), critic 1 (%zu B) and critic 2 (%zu B) + the "
                 "kernel's static LDS (%zu B) exceed the %zu B of LDS of a workgroup", fn, net_bytes[0], net_bytes[1],
                 net_bytes[2], SAC_STATIC_LDS + ACTOR_LDS_SLACK, LDS_PER_WORKGROUP);
        return CTR_EINVAL;
    }
    // ---- ctr_polyak's, and the targets against their online critics
    if (!(u->tau >= 0.f && u->tau <= 1.f)) return ddpg_fail(fn, "tau must be in [0, 1]");
    for (int y = 0; y < 2; ++y)
        if (int r = update_target_check(fn, tk[y], gk[y].net, u->W_targ[y], u->b_targ[y],
                                        "a target critic's shape differs from its online critic's",
                                        "NULL entry in W_targ[2] or b_targ[2]", "NULL layer among W_targ, b_targ [0..n_hidden]"))
            return r;
    // ---- nothing the call writes is anything else it writes or reads (base pointers, as the replaced
    // calls compare them): the aliasing refusals of ctr_td3_critic_step, ctr_sac_actor_step and
    // ctr_polyak, the targets against the online tensors and each other, the blobs, the history
    UpdatePtrs ptrs;
    const int layers[3] = {sk.net.n_hidden + 1, gk[0].net.n_hidden + 1, gk[1].net.n_hidden + 1};
    ptrs.add_net(pp, layers[0]);
    for (int y = 0; y < 2; ++y) ptrs.add_net(ap[y], layers[1 + y]);
    for (int y = 0; y < 2; ++y) ptrs.add_target(u->W_targ[y], u->b_targ[y], layers[1 + y]);
    ptrs.add(ak.blob, "the policy's blob");
    ptrs.add(tk[0].blob, "a target critic's blob");
    ptrs.add(tk[1].blob, "a target critic's blob");
    ptrs.add(u->log_alpha, "log_alpha");
    ptrs.add(al->state, "alpha->state");
    ptrs.add(al->grad, "alpha->grad");
    ptrs.add(u->critic_loss, "critic_loss");
    ptrs.add(u->actor_loss, "actor_loss");
    ptrs.add(u->logp_mean, "logp_mean");
    ptrs.add(u->workspace, "the workspace");
    ptrs.add(u->target, "target");
    ptrs.add(u->q1_next, "q1_next");
    ptrs.add(u->q2_next, "q2_next");
    ptrs.add(u->next_action, "next_action");
    ptrs.add(u->next_logp, "next_logp");
    if (B > 0) ptrs.add_batch(*u->batch);
    ptrs.add(u->history, "history");
    ptrs.add(u->scale, "scale");                                         // (only read)
    if (int r = ptrs.check(fn, u->history, (size_t)updates * 5 * sizeof(float))) return r;
    if (updates == 0 || B == 0) return 0;
    // ---- the launches' arguments, once
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every policy and every critic fit beside the row staging");
    const size_t shm_draw = std::max(ak.bytes, std::max(tk[0].bytes, tk[1].bytes)) + ACTOR_LDS_SLACK;
    size_t shm_td3 = 0;
    for (int y = 0; y < 2; ++y)
        shm_td3 = std::max(shm_td3, ddpg_critic_fill(gk[y], ap[y], u->batch->obs, u->batch->action, u->scale, u->target, B,
                                                     u->critic_loss ? u->critic_loss + y : nullptr));
    if (int r = allow_dynamic_lds(k_her_sample_sac, shm_draw)) return r;
    if (int r = allow_dynamic_lds(k_td3_grad, shm_td3)) return r;
    if (int r = allow_dynamic_lds(k_sac_grad, shm_sac)) return r;
    sk.rows = u->batch->obs;
    sk.log_alpha = u->log_alpha;
    sk.B = (int32_t)B;
    sk.dq = (float)(-1.0 / (double)B);
    sk.inv_B = 1.0 / (double)B;
    ddpg_grad_state(sk, pp);
    sk.lp_part = reinterpret_cast<double *>(sk.ws + lp_off);
    sk.seed = u->seed;
    pp.loss_scale = 1.0 / (double)B;
    pp.loss = u->actor_loss;
    const SacAlphaK alk = {u->log_alpha, al->state, al->grad, u->logp_mean, sk.lp_part, pp.slots,
                           al->learn != 0, 1.0 / (double)B, u->target_entropy, al->lr, pp.beta1, pp.beta2, pp.eps};
    const HerSacK hs = {u->gamma, u->log_alpha, u->target, u->q1_next, u->q2_next, u->next_action, u->next_logp};
    UpdateTailK ct[2], pt = update_tail(pp, ak, nullptr, nullptr, 0, 0.f);
    for (int y = 0; y < 2; ++y) ct[y] = update_tail(ap[y], tk[y], u->W_targ[y], u->b_targ[y], layers[1 + y], u->tau);
    const unsigned gc = grid_for(std::max(tk[0].bytes, tk[1].bytes) / 16), gp = grid_for(ak.bytes / 16);
    const hipStream_t s = (hipStream_t)stream;
    const HerK hk = {*her};
    // the prefix sums of the stored rows, once: nothing below writes the store
    her_scan(her, tiles, stream);
    for (int32_t i = 0; i < updates; ++i) {
        float *hist = u->history ? u->history + 5 * (size_t)i : nullptr;
        ct[0].hist = hist;
        ct[1].hist = hist ? hist + 1 : nullptr;
        pt.hist = hist ? hist + 2 : nullptr;
        sk.counter = u->step_counter + (uint64_t)i;                // both sums are 64-bit and wrap
        hipLaunchKernelGGL(k_her_sample_sac, dim3(grid_for(B)), dim3(BLOCK), shm_draw, s, hk, B, u->draw_seed,
                           u->draw_counter + (uint64_t)i, *u->batch, ak, tk[0], tk[1], hs);
        hipLaunchKernelGGL(k_td3_grad, dim3((unsigned)ap[0].slots, 2), dim3(BLOCK), shm_td3, s, gk[0], gk[1]);
        hipLaunchKernelGGL(k_sac_critic_tail, dim3(gc, 2), dim3(BLOCK), 0, s, ct[0], ct[1]);
        hipLaunchKernelGGL(k_sac_grad, dim3((unsigned)pp.slots), dim3(BLOCK), shm_sac, s, sk);
        hipLaunchKernelGGL(k_sac_policy_tail, dim3(gp), dim3(BLOCK), 0, s, pt, alk, hist);
    }
    return hip_check("ctr_sac_update launch");
}

}  // extern "C"
