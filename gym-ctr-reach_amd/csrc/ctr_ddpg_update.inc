// ctr_ddpg_update.inc -- a run of DDPG or TD3 updates from one call (ctr_ddpg_update;
// include/ctr_reach_amd.h, "A run of DDPG / TD3 updates": the specification).  Included at the end of
// ctr_kernels.hip, after ctr_sac_update.inc.
//
// An update with a policy step is what ctr_her_sample_td (or _td3), ctr_ddpg_critic_step (or
// ctr_td3_critic_step), ctr_ddpg_actor_step, ctr_polyak and ctr_actor_load leave, in five launches:
// the sampler's kernel, the critics' gradient kernel and k_ddpg_grad<true> are launched as those calls
// launch them, and the two kernels here are the tails behind the gradient launches.  An update
// without a policy step (TD3's delay) is the sampler's kernel, the gradient kernel and the existing
// k_ddpg_apply / k_td3_apply.  The sampler's two scans run once per call (the call only reads the store).
//
// A tail does for every parameter of its network what k_ddpg_apply does (the slots' sum in slot order,
// the gradient's store, ddpg_adam), then what k_polyak does (polyak_lerp of the target with the NEW
// online value, the target's store, the target blob's item through actor_item_pack); the actor's tail
// can also pack the online actor's blob item from the new parameters (k_actor_load's work).
//
// Ownership is k_polyak's and k_sac_*_tail's: a workgroup owns BLOCK consecutive 16-B items of the
// blob, and the fragment layout covers every (row, k) once, so every parameter has one owner group
// and the update in place needs no ordering.  The mapping inside the group is not theirs.  There a
// thread owns one item, whose eight weights are two runs of four floats, and neighbouring lanes are
// neighbouring ROWS: every slot is summed from 16-B pieces that lie cols * 4 bytes apart.  Here the
// group's 8 * BLOCK elements are dealt so that a wave's 64 lanes take, in each of eight passes, one
// row of the group's items: lane 16 w + c takes the element of item-wave w (the group's w-th run of 64
// items: one (tile, k-step)) whose column offset in that k-step is c.  Four consecutive k-steps of a
// hidden layer are 64 consecutive columns, so a wave reads 256 contiguous bytes of every slot, of the
// parameter, of m, v and the target, and stores as many; where the group's item-waves are not four
// k-steps of one tile (a 96-wide layer's six k-steps, layer 0, the blob's tail) the runs are the 64 B
// of one item-wave.  Which row and column an (item, j) is comes from actor_item and actor_k_of alone:
// the deal is a bijection of (thread, pass) onto (item, j) whatever the layout, so it decides the
// access pattern and never the result.  The values a blob takes (the new target; the new parameter
// for the online actor) go to LDS, 8 floats per item per blob; behind the group's barrier every
// thread packs its own item from there.
namespace {

static_assert(BLOCK == 256, "the deal below is four waves of 64 lanes over 256 items");

struct DdpgTailK {
    DdpgApplyK ap;
    ActorK ak;                         // the TARGET's layout and blob
    float *Wt[ACTOR_LAYERS], *bt[ACTOR_LAYERS];
    float tau;
    void *online_blob;                 // the actor's tail: the online actor's blob (the target's layout), or NULL
    float *hist;                       // the history row's entry for this network's loss, or NULL
};

// The staging's float4 of item q's half (j >> 2) of a blob's BLOCK items.  Plane `half` holds the
// items' floats 4 half .. 4 half + 3; inside a plane the item's low bits are XORed so that the 32 lanes
// of a store (one row: item-waves w, lane halves h, both j >> 2) fall on all eight 16-B columns of the
// 32 store banks, and the 16 lanes of a ds_read_b128 group (XORed by one constant) stay on 16 columns.
__device__ __forceinline__ int ddpg_tail_slot(int q, int half)
{
    return half * BLOCK + (q ^ (((q >> 5) & 3) | (half << 2)));
}

// A tail's work of one workgroup: items blockIdx.x * BLOCK .. + BLOCK - 1 of k's blob.  s_t, s_p: 8 * BLOCK
// floats each (s_p: ONLINE only).
template <bool ONLINE>
__device__ __forceinline__ void ddpg_tail_group(const DdpgTailK &k, float *s_t, float *s_p)
{
    const DdpgApplyK &a = k.ap;
    const float *hdr = reinterpret_cast<const float *>(a.ws);
    const uint32_t i0 = blockIdx.x * BLOCK, items = k.ak.bytes / 16;
    const float pw1 = hdr[0], pw2 = hdr[1];
    if (i0 + threadIdx.x == 0) {
        // element 0's duties
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
    if (i0 >= items) return;           // (the whole group: a plane past its blob)
    const bool online = ONLINE && k.online_blob != nullptr;
    const float *part = reinterpret_cast<const float *>(a.ws + DDPG_HDR);
    const int64_t stride = ddpg_slot_floats(a.params, a.biases);
    // the deal: this thread's item-wave, lane half and element, and its wave's first row
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int w = lane >> 4, c = lane & 15, h = (c >> 2) & 1, j = 4 * (c >> 3) + (c & 3);
    #pragma unroll 2
    for (int pass = 0; pass < 8; ++pass) {
        const int q = 64 * w + 32 * h + 8 * wave + pass;
        if (i0 + q >= items) continue;
        const ActorItem it = actor_item(k.ak, i0 + q);
        // the element's place in its tensor, or -1: padding (a row, a column or a bias past the layer's)
        int idx = -1;
        if (it.bias) {
            if (j < 4 && it.e + j < it.rows) idx = it.e + j;
        } else if (it.row < it.rows) {
            const int kc = actor_k_of(it.l, it.S, it.h, j);
            if (kc < it.cols) idx = it.row * it.cols + kc;
        }
        float x = 0.f, xp = 0.f;       // what the blobs take: +0 for the padding
        if (idx >= 0) {
            // the item's tensors; the arrays by constant index (they are kernel arguments: a selection
            // by a runtime index becomes a table of the pointers in scratch)
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
            float g;
            if (it.bias) {
                // the slots' f64 sums, rounded once
                const double *bp = reinterpret_cast<const double *>(part + ddpg_slot_w(a.params)) + bo + idx;
                double s = bp[0];
                for (int t = 1; t < a.slots; ++t) s += bp[(size_t)t * (stride / 2)];
                g = (float)s;
            } else {
                const float *wp = part + first + idx;
                g = wp[0];
                #pragma unroll 8
                for (int t = 1; t < a.slots; ++t) g += wp[(size_t)t * stride];
            }
            float m = mp[idx], v = vp[idx];
            const float told = tp[idx];
            gp[idx] = g;
            xp = ddpg_adam(p[idx], g, m, v, a.lr, a.beta1, a.beta2, a.eps, pw1, pw2);
            p[idx] = xp;
            mp[idx] = m;
            vp[idx] = v;
            x = polyak_lerp(told, xp, k.tau);
            tp[idx] = x;
        }
        const int s = 4 * ddpg_tail_slot(q, j >> 2) + (j & 3);
        s_t[s] = x;
        if (online) s_p[s] = xp;
    }
    __syncthreads();
    // every thread packs its own item from the staging
    const int q = (int)threadIdx.x;
    if (i0 + q >= items) return;
    const ActorItem it = actor_item(k.ak, i0 + q);
    const float4 lo = *reinterpret_cast<const float4 *>(s_t + 4 * ddpg_tail_slot(q, 0));
    const float4 hi = *reinterpret_cast<const float4 *>(s_t + 4 * ddpg_tail_slot(q, 1));
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    static_cast<uint4 *>(const_cast<void *>(k.ak.blob))[i0 + q] = actor_item_pack(it, v);
    if (online) {
        const float4 plo = *reinterpret_cast<const float4 *>(s_p + 4 * ddpg_tail_slot(q, 0));
        const float4 phi = *reinterpret_cast<const float4 *>(s_p + 4 * ddpg_tail_slot(q, 1));
        const float vp[8] = {plo.x, plo.y, plo.z, plo.w, phi.x, phi.y, phi.z, phi.w};
        static_cast<uint4 *>(k.online_blob)[i0 + q] = actor_item_pack(it, vp);
    }
}

// The critics' tail: plane blockIdx.y works on critic y and its target (the grid's x is the larger
// blob's; a plane's groups past its blob leave).
__global__ __launch_bounds__(BLOCK) void k_ddpg_critic_tail(DdpgTailK k0, DdpgTailK k1)
{
    __shared__ __attribute__((aligned(16))) float s_t[8 * BLOCK];
    if (blockIdx.y == 0) ddpg_tail_group<false>(k0, s_t, nullptr);
    else ddpg_tail_group<false>(k1, s_t, nullptr);
}

// The policy's tail: the policy and the target policy, and the online actor's blob when there is one.
__global__ __launch_bounds__(BLOCK) void k_ddpg_actor_tail(DdpgTailK k)
{
    __shared__ __attribute__((aligned(16))) float s_t[8 * BLOCK];
    __shared__ __attribute__((aligned(16))) float s_p[8 * BLOCK];
    ddpg_tail_group<true>(k, s_t, s_p);
}

// The critic losses of a call's last update into its history row, where that update made no policy
// step (k_ddpg_apply / k_td3_apply have one loss output).
__global__ __launch_bounds__(64) void k_ddpg_loss_copy(const float *loss, float *hist, int n)
{
    if ((int)threadIdx.x < n) hist[threadIdx.x] = loss[threadIdx.x];
}

int ddpg_update_fail(const char *a, const char *b)
{
    snprintf(g_err, sizeof g_err, "ctr_ddpg_update: %s and %s are the same memory", a, b);
    return CTR_EINVAL;
}

// A target's layout against its online network's shape.
bool ddpg_same_shape(const ActorK &t, const DdpgNetK &n)
{
    bool same = t.in_dim == n.in_dim && t.n_hidden == n.n_hidden;
    for (int l = 0; same && l < n.n_hidden; ++l) same = 32 * t.tiles[l] == n.width[l];
    return same;
}

}  // namespace

extern "C" {

int ctr_ddpg_update(const ctr_ddpg_update_t *u, int32_t updates, void *stream)
{
    const char *fn = "ctr_ddpg_update";
    if (!u) return ddpg_fail(fn, "u is NULL");
    if (updates < 0) return ddpg_fail(fn, "updates must be >= 0");
    const int nc = u->n_critics;
    if (nc < 1 || nc > 2) return ddpg_fail(fn, "n_critics must be 1 (DDPG) or 2 (TD3)");
    if (u->policy_delay < 1) return ddpg_fail(fn, "policy_delay must be >= 1");
    const int64_t B = u->batch_size;
    // ---- ctr_her_sample_td's / ctr_her_sample_td3's checks
    int64_t tiles = 0;
    if (int r = td_named(fn, her_sample_check(fn, u->her, B, u->batch, &tiles))) return r;
    ActorK atk, tk[2] = {}, ok = {};
    if (int r = td_named(fn, actor_layout(u->actor_targ, &atk))) return r;        // (the scale is not read)
    if (int r = td_named(fn, mlp_blob("actor", u->actor_targ->blob, &atk))) return r;
    for (int y = 0; y < nc; ++y) {
        if (!u->critic_targ[y]) return ddpg_fail(fn, "NULL entry in critic_targ[n_critics]");
        if (int r = td_named(fn, critic_check(u->critic_targ[y], &tk[y]))) return r;
    }
    const ctr_her_t *her = u->her;
    if (atk.in_dim != her->obs_dim + 6) return ddpg_fail(fn, "actor_targ->in_dim must be her->obs_dim + 6");
    for (int y = 0; y < nc; ++y)
        if (tk[y].in_dim != her->obs_dim + 12) return ddpg_fail(fn, "a critic_targ's in_dim must be her->obs_dim + 12");
    if (!isfinite(u->gamma)) return ddpg_fail(fn, "gamma must be finite");
    if (nc == 2) {
        if (!isfinite(u->sigma) || u->sigma < 0.f) return ddpg_fail(fn, "sigma must be finite and >= 0");
        if (!(u->clip >= 0.f)) return ddpg_fail(fn, "clip must be >= 0 (INFINITY: no clip)");
    }
    if (!u->target) return ddpg_fail(fn, "target is NULL");
    // ---- ctr_ddpg_critic_step's / ctr_td3_critic_step's, on the batch's obs, action and the target
    DdpgGradK gk[2] = {};
    DdpgApplyK ap[2] = {};
    for (int y = 0; y < nc; ++y) {
        if (!u->critic[y] || !u->critic_net[y]) return ddpg_fail(fn, "NULL entry in critic[n_critics] or critic_net[n_critics]");
        if (int r = ddpg_shape_check(fn, nullptr, u->critic[y], false, nullptr, &gk[y].net)) return r;
    }
    if (nc == 2 && gk[0].net.in_dim != gk[1].net.in_dim) return ddpg_fail(fn, "the two critics must have the same in_dim");
    const int64_t Bc = std::min(B, DDPG_MAX_B);
    const int64_t off = ddpg_ws_bytes(gk[0].net.params, gk[0].net.biases, Bc);
    if (int r = ddpg_learn_check(fn, u->critic_net[0], u->critic_adam, B, u->workspace, u->workspace_bytes, &gk[0].net, &ap[0]))
        return r;
    if (nc == 2) {
        if (u->workspace_bytes < off + ddpg_ws_bytes(gk[1].net.params, gk[1].net.biases, Bc))
            return ddpg_fail(fn, "workspace too small (ctr_td3_workspace_bytes)");
        if (int r = ddpg_learn_check(fn, u->critic_net[1], u->critic_adam, B, static_cast<char *>(u->workspace) + off,
                                     u->workspace_bytes - off, &gk[1].net, &ap[1]))
            return r;
    }
    // ---- ctr_ddpg_actor_step's, on the batch's obs under critic 0
    DdpgGradK pg = {};
    DdpgApplyK pp;
    if (int r = ddpg_shape_check(fn, u->policy, u->critic[0], true, &pg.net, &pg.crit)) return r;
    if (int r = ddpg_learn_check(fn, u->policy_net, u->policy_adam, B, u->workspace, u->workspace_bytes, &pg.net, &pp)) return r;
    for (int l = 0; l <= pg.crit.n_hidden; ++l) {
        pg.crit.W[l] = gk[0].net.W[l];
        pg.crit.b[l] = gk[0].net.b[l];
    }
    // ---- ctr_polyak's, the targets against their online networks, ctr_actor_load's
    if (!(u->tau >= 0.f && u->tau <= 1.f)) return ddpg_fail(fn, "tau must be in [0, 1]");
    if (!ddpg_same_shape(atk, pg.net)) return ddpg_fail(fn, "the target policy's shape differs from the policy's");
    if (!u->W_targ_actor || !u->b_targ_actor) return ddpg_fail(fn, "W_targ_actor or b_targ_actor is NULL");
    for (int l = 0; l <= pg.net.n_hidden; ++l)
        if (!u->W_targ_actor[l] || !u->b_targ_actor[l])
            return ddpg_fail(fn, "NULL layer among W_targ_actor, b_targ_actor [0..n_hidden]");
    for (int y = 0; y < nc; ++y) {
        const DdpgNetK &cn = gk[y].net;
        if (!ddpg_same_shape(tk[y], cn)) return ddpg_fail(fn, "a target critic's shape differs from its online critic's");
        if (!u->W_targ[y] || !u->b_targ[y]) return ddpg_fail(fn, "NULL entry in W_targ[n_critics] or b_targ[n_critics]");
        for (int l = 0; l <= cn.n_hidden; ++l)
            if (!u->W_targ[y][l] || !u->b_targ[y][l]) return ddpg_fail(fn, "NULL layer among W_targ, b_targ [0..n_hidden]");
    }
    if (u->actor) {
        if (int r = td_named(fn, actor_layout(u->actor, &ok))) return r;
        if (int r = td_named(fn, mlp_blob("actor", u->actor->blob, &ok))) return r;
        if (!ddpg_same_shape(ok, pg.net)) return ddpg_fail(fn, "the online actor's shape differs from the policy's");
    }
    // ---- nothing the call writes is anything else it writes or reads (base pointers, as the replaced
    // calls compare them)
    static const char *const tn[4] = {"a parameter tensor", "a gradient tensor", "a first-moment tensor", "a second-moment tensor"};
    SacPtr ptr[3 * (4 * DDPG_TENSORS + 1) + 3 * DDPG_TENSORS + 32];
    int np = 0;
    auto add = [&](const void *p, const char *name, bool written) {
        if (p) ptr[np++] = SacPtr{p, name, written};
    };
    const DdpgApplyK *const nets[3] = {&pp, &ap[0], &ap[1]};
    const int layers[3] = {pg.net.n_hidden + 1, gk[0].net.n_hidden + 1, gk[1].net.n_hidden + 1};
    for (int n = 0; n < 1 + nc; ++n) {
        for (int t = 0; t < 2 * layers[n]; ++t) {
            add(nets[n]->p[t], tn[0], true);
            add(nets[n]->g[t], tn[1], true);
            add(nets[n]->m[t], tn[2], true);
            add(nets[n]->v[t], tn[3], true);
        }
        add(nets[n]->pow, "a net's pow", true);
    }
    for (int l = 0; l < layers[0]; ++l) {
        add(u->W_targ_actor[l], "a target tensor", true);
        add(u->b_targ_actor[l], "a target tensor", true);
    }
    for (int y = 0; y < nc; ++y)
        for (int l = 0; l < layers[1 + y]; ++l) {
            add(u->W_targ[y][l], "a target tensor", true);
            add(u->b_targ[y][l], "a target tensor", true);
        }
    add(atk.blob, "the target policy's blob", true);
    for (int y = 0; y < nc; ++y) add(tk[y].blob, "a target critic's blob", true);
    add(ok.blob, "the online actor's blob", true);
    add(u->critic_loss, "critic_loss", true);
    add(u->actor_loss, "actor_loss", true);
    add(u->workspace, "the workspace", true);
    add(u->target, "target", true);
    add(u->q1_next, "q1_next", true);
    if (nc == 2) add(u->q2_next, "q2_next", true);
    add(u->next_action, "next_action", true);
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
        if (ptr[i].p == ptr[i + 1].p) return ddpg_update_fail(ptr[i].name, ptr[i + 1].name);
    const int hcols = 1 + nc;
    if (u->history) {
        const char *h0 = reinterpret_cast<const char *>(u->history), *h1 = h0 + (size_t)updates * hcols * sizeof(float);
        for (int i = 0; i < np; ++i)
            if (ptr[i].p != u->history && (const char *)ptr[i].p >= h0 && (const char *)ptr[i].p < h1)
                return ddpg_update_fail("history", ptr[i].name);
    }
    if (updates == 0 || B == 0) return 0;
    // ---- the launches' arguments, once
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every actor and every critic fit beside the row staging");
    const size_t shm_draw = std::max(atk.bytes, std::max(tk[0].bytes, tk[1].bytes)) + ACTOR_LDS_SLACK;
    size_t shm_critic = 0;
    for (int y = 0; y < nc; ++y) {
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
        shm_critic = std::max(shm_critic, ddpg_lds_floats(gk[y].net) * sizeof(float) + ACTOR_LDS_SLACK);
    }
    const size_t shm_actor = (ddpg_lds_floats(pg.net) + ddpg_lds_floats(pg.crit)) * sizeof(float) + ACTOR_LDS_SLACK;
    if (nc == 1) {
        if (int r = allow_dynamic_lds(k_her_sample_td, shm_draw)) return r;
        if (int r = allow_dynamic_lds(k_ddpg_grad<false>, shm_critic)) return r;
    } else {
        if (int r = allow_dynamic_lds(k_her_sample_td3, shm_draw)) return r;
        if (int r = allow_dynamic_lds(k_td3_grad, shm_critic)) return r;
    }
    if (int r = allow_dynamic_lds(k_ddpg_grad<true>, shm_actor)) return r;
    pg.rows = u->batch->obs;
    pg.B = (int32_t)B;
    pg.dq = (float)(-1.0 / (double)B);
    pg.beta1 = pp.beta1;
    pg.beta2 = pp.beta2;
    pg.pow = pp.pow;
    pg.ws = const_cast<char *>(pp.ws);
    pp.loss_scale = -1.0 / (double)B;
    pp.loss = u->actor_loss;
    const TdK td1 = {u->gamma, u->target, u->q1_next, u->next_action};
    const Td3K td2 = {u->gamma, u->sigma, u->clip, u->target, u->q1_next, u->q2_next, u->next_action};
    DdpgTailK ct[2] = {}, pt = {};
    for (int y = 0; y < nc; ++y) {
        ct[y].ap = ap[y];
        ct[y].ak = tk[y];
        for (int l = 0; l < layers[1 + y]; ++l) {
            ct[y].Wt[l] = u->W_targ[y][l];
            ct[y].bt[l] = u->b_targ[y][l];
        }
        ct[y].tau = u->tau;
    }
    pt.ap = pp;
    pt.ak = atk;
    for (int l = 0; l < layers[0]; ++l) {
        pt.Wt[l] = u->W_targ_actor[l];
        pt.bt[l] = u->b_targ_actor[l];
    }
    pt.tau = u->tau;
    pt.online_blob = const_cast<void *>(ok.blob);
    const unsigned gc = grid_for(std::max(tk[0].bytes, tk[1].bytes) / 16), gp = grid_for(atk.bytes / 16);
    const unsigned ga = grid_for(std::max(ap[0].params, ap[1].params));
    const unsigned slots = (unsigned)ap[0].slots;
    const hipStream_t s = (hipStream_t)stream;
    const HerK hk = {*her};
    // the prefix sums of the stored rows, once: nothing below writes the store
    hipLaunchKernelGGL(k_her_scan_tiles, dim3((unsigned)tiles), dim3(BLOCK), 0, s, hk);
    hipLaunchKernelGGL(k_her_scan_tops, dim3(1), dim3(BLOCK), 0, s, hk, tiles);
    bool copy_last = false;
    for (int32_t i = 0; i < updates; ++i) {
        float *hist = u->history ? u->history + (size_t)hcols * (size_t)i : nullptr;
        const uint64_t counter = u->draw_counter + (uint64_t)i;             // a 64-bit sum that wraps
        const bool step = (u->update_index + (uint64_t)i + 1) % (uint64_t)u->policy_delay == 0;
        if (nc == 1) {
            hipLaunchKernelGGL(k_her_sample_td, dim3(grid_for(B)), dim3(BLOCK), shm_draw, s, hk, B, u->draw_seed, counter,
                               *u->batch, atk, tk[0], td1);
            hipLaunchKernelGGL(k_ddpg_grad<false>, dim3(slots), dim3(BLOCK), shm_critic, s, gk[0]);
        } else {
            hipLaunchKernelGGL(k_her_sample_td3, dim3(grid_for(B)), dim3(BLOCK), shm_draw, s, hk, B, u->draw_seed, counter,
                               *u->batch, atk, tk[0], tk[1], td2);
            hipLaunchKernelGGL(k_td3_grad, dim3(slots, 2), dim3(BLOCK), shm_critic, s, gk[0], gk[1]);
        }
        if (step) {
            ct[0].hist = hist;
            ct[1].hist = hist ? hist + 1 : nullptr;
            pt.hist = hist ? hist + nc : nullptr;
            hipLaunchKernelGGL(k_ddpg_critic_tail, dim3(gc, (unsigned)nc), dim3(BLOCK), 0, s, ct[0], ct[1]);
            hipLaunchKernelGGL(k_ddpg_grad<true>, dim3((unsigned)pp.slots), dim3(BLOCK), shm_actor, s, pg);
            hipLaunchKernelGGL(k_ddpg_actor_tail, dim3(gp), dim3(BLOCK), 0, s, pt);
            continue;
        }
        // no policy step: the critics' apply kernel as it is.  It has one loss output: the history row's
        // entries, but for the call's last update, whose losses critic_loss keeps (an earlier update's
        // would be overwritten in stream order anyway)
        DdpgApplyK la[2] = {ap[0], ap[1]};
        const bool last = i == updates - 1;
        if (hist && !(last && u->critic_loss)) {
            la[0].loss = hist;
            la[1].loss = hist + 1;
        }
        copy_last = last && hist && u->critic_loss;
        if (nc == 1) hipLaunchKernelGGL(k_ddpg_apply, dim3(ga), dim3(BLOCK), 0, s, la[0]);
        else hipLaunchKernelGGL(k_td3_apply, dim3(ga, 2), dim3(BLOCK), 0, s, la[0], la[1]);
    }
    // ... and that update's history entries are copied from there
    if (copy_last)
        hipLaunchKernelGGL(k_ddpg_loss_copy, dim3(1), dim3(64), 0, s, u->critic_loss,
                           u->history + (size_t)hcols * (size_t)(updates - 1), nc);
    return hip_check("ctr_ddpg_update launch");
}

}  // extern "C"
