// ctr_sac_update.inc -- a run of SAC updates from one call (ctr_sac_update; include/ctr_reach_amd.h,
// "A run of SAC updates": the specification).  Included at the end of ctr_kernels.hip, after
// ctr_sac.inc and ctr_polyak.inc.
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

// What a tail takes: the apply launch's arguments, the blob's layout (ak.blob: the blob written),
// and for the critics the target's tensors.
struct SacTailK {
    DdpgApplyK ap;
    ActorK ak;
    float *Wt[ACTOR_LAYERS], *bt[ACTOR_LAYERS];
    float tau;
    float *hist;                       // the history row's entry for this network's loss, or NULL
};

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

// ddpg_apply_element's work on the run's elements of tensor `tensor` (its first flat element: first;
// a bias: its first double among a slot's bias sums: bo), and the LERP of the target's.  x: the new
// values the blob item packs (the target's with LERP, else the parameters'); past n: +0.
template <bool LERP>
__device__ __forceinline__ void sac_tail_run(const SacTailK &k, const SacRun &r, int tensor, int first, int bo, float *p,
                                             float *gp, float *mp, float *vp, float *tp, float pw1, float pw2, float x[4])
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
        const double *bp = reinterpret_cast<const double *>(part + ddpg_slot_w(a.params)) + bo + r.i;
        #pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < r.n) {
                double s = bp[j];
                for (int t = 1; t < a.slots; ++t) s += bp[(size_t)t * (stride / 2) + j];
                g[j] = (float)s;
            }
    } else {
        const SacRun rs = {first + r.i, r.n, r.vec};
        sac_run_load(part, rs, g);
        for (int t = 1; t < a.slots; ++t) {
            float q[4];
            sac_run_load(part + (size_t)t * stride, rs, q);
            #pragma unroll
            for (int j = 0; j < 4; ++j) g[j] += q[j];
        }
    }
    float pv[4], m[4], v[4], tv[4] = {0.f, 0.f, 0.f, 0.f};
    sac_run_load(p, r, pv);
    sac_run_load(mp, r, m);
    sac_run_load(vp, r, v);
    if (LERP) sac_run_load(tp, r, tv);
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < r.n) {
            pv[j] = ddpg_adam(pv[j], g[j], m[j], v[j], a.lr, a.beta1, a.beta2, a.eps, pw1, pw2);
            if (LERP) tv[j] = polyak_lerp(tv[j], pv[j], k.tau);
        }
        x[j] = j < r.n ? (LERP ? tv[j] : pv[j]) : 0.f;
    }
    sac_run_store(gp, r, g);
    sac_run_store(p, r, pv);
    sac_run_store(mp, r, m);
    sac_run_store(vp, r, v);
    if (LERP) sac_run_store(tp, r, tv);
}

// A tail's work of one thread: item blockIdx.x * BLOCK + threadIdx.x of k's blob.
template <bool LERP>
__device__ __forceinline__ void sac_tail_item(const SacTailK &k)
{
    const DdpgApplyK &a = k.ap;
    const float *hdr = reinterpret_cast<const float *>(a.ws);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const float pw1 = hdr[0], pw2 = hdr[1];
    if (i == 0) {
        a.pow[0] = pw1;
        a.pow[1] = pw2;
        if (a.loss || k.hist) {
            const double *lpart = reinterpret_cast<const double *>(a.ws + 16);
            double s = lpart[0];
            for (int t = 1; t < a.slots; ++t) s += lpart[t];
            const float loss = (float)(s * a.loss_scale);
            if (a.loss) *a.loss = loss;
            if (k.hist) *k.hist = loss;
        }
    }
    if (i >= k.ak.bytes / 16) return;
    const ActorItem it = actor_item(k.ak, i);
    // the item's tensor; the arrays by constant index (they are kernel arguments)
    const int tensor = 2 * it.l + (it.bias ? 1 : 0);
    // (per layer, as k_actor_load and k_polyak select theirs: a selection by the tensor's index 0..7
    // becomes a table of the pointers in scratch)
    int first = 0, bo = a.boff[0];
    float *p = a.p[0], *gp = a.g[0], *mp = a.m[0], *vp = a.v[0], *tp = k.Wt[0];
    #pragma unroll
    for (int l = 0; l < ACTOR_LAYERS; ++l)
        if (it.l == l) {
            first = it.bias ? a.end[2 * l] : (l ? a.end[l ? 2 * l - 1 : 0] : 0);
            bo = a.boff[l];
            p = it.bias ? a.p[2 * l + 1] : a.p[2 * l];
            gp = it.bias ? a.g[2 * l + 1] : a.g[2 * l];
            mp = it.bias ? a.m[2 * l + 1] : a.m[2 * l];
            vp = it.bias ? a.v[2 * l + 1] : a.v[2 * l];
            tp = it.bias ? k.bt[l] : k.Wt[l];
        }
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
    sac_tail_run<LERP>(k, r[0], tensor, first, bo, p, gp, mp, vp, tp, pw1, pw2, v);
    sac_tail_run<LERP>(k, r[1], tensor, first, bo, p, gp, mp, vp, tp, pw1, pw2, v + 4);
    static_cast<uint4 *>(const_cast<void *>(k.ak.blob))[i] = actor_item_pack(it, v);
}

// The critics' tail: plane blockIdx.y works on critic y and its target (the grid's x is the larger
// blob's; the threads past a blob's items leave).
__global__ __launch_bounds__(BLOCK) void k_sac_critic_tail(SacTailK k0, SacTailK k1)
{
    if (blockIdx.y == 0) sac_tail_item<true>(k0);
    else sac_tail_item<true>(k1);
}

// The policy's tail; the grid's last thread makes the temperature's step as k_sac_apply's does, and
// writes the history row's logp_mean and log_alpha.
__global__ __launch_bounds__(BLOCK) void k_sac_policy_tail(SacTailK k, SacAlphaK a, float *hist)
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

// A pointer the call writes through (or, read: only reads), with its name for the message.
struct SacPtr {
    const void *p;
    const char *name;
    bool written;
};

int sac_update_fail(const char *a, const char *b)
{
    snprintf(g_err, sizeof g_err, "ctr_sac_update: %s and %s are the same memory", a, b);
    return CTR_EINVAL;
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
    if (!u->critic[0] || !u->critic[1] || !u->critic_net[0] || !u->critic_net[1])
        return ddpg_fail(fn, "NULL entry in critic[2] or critic_net[2]");
    if (int r = ddpg_shape_check(fn, nullptr, u->critic[0], false, nullptr, &gk[0].net)) return r;
    if (int r = ddpg_shape_check(fn, nullptr, u->critic[1], false, nullptr, &gk[1].net)) return r;
    if (gk[0].net.in_dim != gk[1].net.in_dim) return ddpg_fail(fn, "the two critics must have the same in_dim");
    const int64_t Bc = std::min(B, DDPG_MAX_B);
    const int64_t off = ddpg_ws_bytes(gk[0].net.params, gk[0].net.biases, Bc);
    if (int r = ddpg_learn_check(fn, u->critic_net[0], u->critic_adam, B, u->workspace, u->workspace_bytes, &gk[0].net, &ap[0]))
        return r;
    if (u->workspace_bytes < off + ddpg_ws_bytes(gk[1].net.params, gk[1].net.biases, Bc))
        return ddpg_fail(fn, "workspace too small (ctr_sac_workspace_bytes)");
    if (int r = ddpg_learn_check(fn, u->critic_net[1], u->critic_adam, B, static_cast<char *>(u->workspace) + off,
                                 u->workspace_bytes - off, &gk[1].net, &ap[1]))
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
    for (int y = 0; y < 2; ++y) {
        const DdpgNetK &cn = gk[y].net;
        bool same = tk[y].in_dim == cn.in_dim && tk[y].n_hidden == cn.n_hidden;
        for (int l = 0; same && l < cn.n_hidden; ++l) same = 32 * tk[y].tiles[l] == cn.width[l];
        if (!same) return ddpg_fail(fn, "a target critic's shape differs from its online critic's");
        if (!u->W_targ[y] || !u->b_targ[y]) return ddpg_fail(fn, "NULL entry in W_targ[2] or b_targ[2]");
        for (int l = 0; l <= cn.n_hidden; ++l)
            if (!u->W_targ[y][l] || !u->b_targ[y][l]) return ddpg_fail(fn, "NULL layer among W_targ, b_targ [0..n_hidden]");
    }
    // ---- nothing the call writes is anything else it writes or reads (base pointers, as the replaced
    // calls compare them): the aliasing refusals of ctr_td3_critic_step, ctr_sac_actor_step and
    // ctr_polyak, the targets against the online tensors and each other, the blobs, the history
    static const char *const tn[4] = {"a parameter tensor", "a gradient tensor", "a first-moment tensor", "a second-moment tensor"};
    SacPtr ptr[3 * (4 * DDPG_TENSORS + 1) + 2 * DDPG_TENSORS + 32];
    int np = 0;
    auto add = [&](const void *p, const char *name, bool written) {
        if (p) ptr[np++] = SacPtr{p, name, written};
    };
    const DdpgApplyK *const nets[3] = {&pp, &ap[0], &ap[1]};
    const int layers[3] = {sk.net.n_hidden + 1, gk[0].net.n_hidden + 1, gk[1].net.n_hidden + 1};
    for (int n = 0; n < 3; ++n) {
        for (int t = 0; t < 2 * layers[n]; ++t) {
            add(nets[n]->p[t], tn[0], true);
            add(nets[n]->g[t], tn[1], true);
            add(nets[n]->m[t], tn[2], true);
            add(nets[n]->v[t], tn[3], true);
        }
        add(nets[n]->pow, "a net's pow", true);
    }
    for (int y = 0; y < 2; ++y)
        for (int l = 0; l < layers[1 + y]; ++l) {
            add(u->W_targ[y][l], "a target tensor", true);
            add(u->b_targ[y][l], "a target tensor", true);
        }
    add(ak.blob, "the policy's blob", true);
    add(tk[0].blob, "a target critic's blob", true);
    add(tk[1].blob, "a target critic's blob", true);
    add(u->log_alpha, "log_alpha", true);
    add(al->state, "alpha->state", true);
    add(al->grad, "alpha->grad", true);
    add(u->critic_loss, "critic_loss", true);
    add(u->actor_loss, "actor_loss", true);
    add(u->logp_mean, "logp_mean", true);
    add(u->workspace, "the workspace", true);
    add(u->target, "target", true);
    add(u->q1_next, "q1_next", true);
    add(u->q2_next, "q2_next", true);
    add(u->next_action, "next_action", true);
    add(u->next_logp, "next_logp", true);
    if (B > 0) {
        add(u->batch->obs, "batch->obs", true);
        add(u->batch->action, "batch->action", true);
        add(u->batch->reward, "batch->reward", true);
        add(u->batch->next_obs, "batch->next_obs", true);
        add(u->batch->done, "batch->done", true);
        add(u->batch->index, "batch->index", true);
    }
    add(u->history, "history", true);
    add(u->scale, "scale", false);
    std::sort(ptr, ptr + np, [](const SacPtr &a, const SacPtr &b) { return (uintptr_t)a.p < (uintptr_t)b.p; });
    for (int i = 0; i + 1 < np; ++i)
        if (ptr[i].p == ptr[i + 1].p) return sac_update_fail(ptr[i].name, ptr[i + 1].name);
    if (u->history) {
        const char *h0 = reinterpret_cast<const char *>(u->history), *h1 = h0 + (size_t)updates * 5 * sizeof(float);
        for (int i = 0; i < np; ++i)
            if (ptr[i].p != u->history && (const char *)ptr[i].p >= h0 && (const char *)ptr[i].p < h1)
                return sac_update_fail("history", ptr[i].name);
    }
    if (updates == 0 || B == 0) return 0;
    // ---- the launches' arguments, once
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every policy and every critic fit beside the row staging");
    const size_t shm_draw = std::max(ak.bytes, std::max(tk[0].bytes, tk[1].bytes)) + ACTOR_LDS_SLACK;
    size_t shm_td3 = 0;
    for (int y = 0; y < 2; ++y) {
        gk[y].rows = u->batch->obs;
        gk[y].actions = u->batch->action;
        gk[y].scale = u->scale;
        gk[y].target = u->target;
        gk[y].B = (int32_t)B;
        gk[y].dq = (float)(2.0 / (double)B);
        gk[y].beta1 = ap[y].beta1;
        gk[y].beta2 = ap[y].beta2;
        gk[y].pow = ap[y].pow;
        gk[y].ws = const_cast<char *>(ap[y].ws);
        ap[y].loss_scale = 1.0 / (double)B;
        ap[y].loss = u->critic_loss ? u->critic_loss + y : nullptr;
        shm_td3 = std::max(shm_td3, ddpg_lds_floats(gk[y].net) * sizeof(float) + ACTOR_LDS_SLACK);
    }
    if (int r = allow_dynamic_lds(k_her_sample_sac, shm_draw)) return r;
    if (int r = allow_dynamic_lds(k_td3_grad, shm_td3)) return r;
    if (int r = allow_dynamic_lds(k_sac_grad, shm_sac)) return r;
    sk.rows = u->batch->obs;
    sk.log_alpha = u->log_alpha;
    sk.B = (int32_t)B;
    sk.dq = (float)(-1.0 / (double)B);
    sk.inv_B = 1.0 / (double)B;
    sk.beta1 = pp.beta1;
    sk.beta2 = pp.beta2;
    sk.pow = pp.pow;
    sk.ws = const_cast<char *>(pp.ws);
    sk.lp_part = reinterpret_cast<double *>(sk.ws + lp_off);
    sk.seed = u->seed;
    pp.loss_scale = 1.0 / (double)B;
    pp.loss = u->actor_loss;
    const SacAlphaK alk = {u->log_alpha, al->state, al->grad, u->logp_mean, sk.lp_part, pp.slots,
                           al->learn != 0, 1.0 / (double)B, u->target_entropy, al->lr, pp.beta1, pp.beta2, pp.eps};
    const HerSacK hs = {u->gamma, u->log_alpha, u->target, u->q1_next, u->q2_next, u->next_action, u->next_logp};
    SacTailK ct[2] = {}, pt = {};
    for (int y = 0; y < 2; ++y) {
        ct[y].ap = ap[y];
        ct[y].ak = tk[y];
        for (int l = 0; l < layers[1 + y]; ++l) {
            ct[y].Wt[l] = u->W_targ[y][l];
            ct[y].bt[l] = u->b_targ[y][l];
        }
        ct[y].tau = u->tau;
    }
    pt.ap = pp;
    pt.ak = ak;
    const unsigned gc = grid_for(std::max(tk[0].bytes, tk[1].bytes) / 16), gp = grid_for(ak.bytes / 16);
    const hipStream_t s = (hipStream_t)stream;
    const HerK hk = {*her};
    // the prefix sums of the stored rows, once: nothing below writes the store
    hipLaunchKernelGGL(k_her_scan_tiles, dim3((unsigned)tiles), dim3(BLOCK), 0, s, hk);
    hipLaunchKernelGGL(k_her_scan_tops, dim3(1), dim3(BLOCK), 0, s, hk, tiles);
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
