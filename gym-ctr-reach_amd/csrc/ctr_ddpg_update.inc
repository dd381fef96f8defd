// ctr_ddpg_update.inc -- a run of DDPG or TD3 updates from one call (ctr_ddpg_update;
// include/ctr_reach_amd.h, "A run of DDPG / TD3 updates": the specification).  Included at the end of
// ctr_kernels.hip, after ctr_update_common.inc (the tails' arguments and tensor selection, the host checks
// both update calls share) and ctr_sac_update.inc.
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
    UpdateTailK t;                     // (t.ak: the TARGET's layout and blob)
    void *online_blob;                 // the actor's tail: the online actor's blob (the target's layout), or NULL
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
__device__ __forceinline__ void ddpg_tail_group(const DdpgTailK &kd, float *s_t, float *s_p)
{
    const UpdateTailK &k = kd.t;
    const DdpgApplyK &a = k.ap;
    const float *hdr = reinterpret_cast<const float *>(a.ws);
    const uint32_t i0 = blockIdx.x * BLOCK, items = k.ak.bytes / 16;
    const float pw1 = hdr[0], pw2 = hdr[1];
    if (i0 + threadIdx.x == 0) ddpg_apply_head(a, k.hist, pw1, pw2);
    if (i0 >= items) return;           // (the whole group: a plane past its blob)
    const bool online = ONLINE && kd.online_blob != nullptr;
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
            const UpdateTensors ts = update_tensors(k, it);
            float g;
            if (it.bias) {
                // the slots' f64 sums, rounded once
                const double *bp = reinterpret_cast<const double *>(part + ddpg_slot_w(a.params)) + ts.bo + idx;
                double s = bp[0];
                for (int t = 1; t < a.slots; ++t) s += bp[(size_t)t * (stride / 2)];
                g = (float)s;
            } else {
                const float *wp = part + ts.first + idx;
                g = wp[0];
                #pragma unroll 8
                for (int t = 1; t < a.slots; ++t) g += wp[(size_t)t * stride];
            }
            float m = ts.mp[idx], v = ts.vp[idx];
            const float told = ts.tp[idx];
            ts.gp[idx] = g;
            xp = ddpg_adam(ts.p[idx], g, m, v, a.lr, a.beta1, a.beta2, a.eps, pw1, pw2);
            ts.p[idx] = xp;
            ts.mp[idx] = m;
            ts.vp[idx] = v;
            x = polyak_lerp(told, xp, k.tau);
            ts.tp[idx] = x;
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
        static_cast<uint4 *>(kd.online_blob)[i0 + q] = actor_item_pack(it, vp);
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
    if (int r = ddpg_critics_check(fn, nc, u->critic, u->critic_net, u->critic_adam, B, u->workspace, u->workspace_bytes,
                                   "NULL entry in critic[n_critics] or critic_net[n_critics]",
                                   "workspace too small (ctr_td3_workspace_bytes)", gk, ap))
        return r;
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
    if (int r = update_target_check(fn, atk, pg.net, u->W_targ_actor, u->b_targ_actor,
                                    "the target policy's shape differs from the policy's", "W_targ_actor or b_targ_actor is NULL",
                                    "NULL layer among W_targ_actor, b_targ_actor [0..n_hidden]"))
        return r;
    for (int y = 0; y < nc; ++y)
        if (int r = update_target_check(fn, tk[y], gk[y].net, u->W_targ[y], u->b_targ[y],
                                        "a target critic's shape differs from its online critic's",
                                        "NULL entry in W_targ[n_critics] or b_targ[n_critics]",
                                        "NULL layer among W_targ, b_targ [0..n_hidden]"))
            return r;
    if (u->actor) {
        if (int r = td_named(fn, actor_layout(u->actor, &ok))) return r;
        if (int r = td_named(fn, mlp_blob("actor", u->actor->blob, &ok))) return r;
        if (!ddpg_same_shape(ok, pg.net)) return ddpg_fail(fn, "the online actor's shape differs from the policy's");
    }
    // ---- nothing the call writes is anything else it writes or reads (base pointers, as the replaced
    // calls compare them)
    UpdatePtrs ptrs;
    const int layers[3] = {pg.net.n_hidden + 1, gk[0].net.n_hidden + 1, gk[1].net.n_hidden + 1};
    ptrs.add_net(pp, layers[0]);
    for (int y = 0; y < nc; ++y) ptrs.add_net(ap[y], layers[1 + y]);
    ptrs.add_target(u->W_targ_actor, u->b_targ_actor, layers[0]);
    for (int y = 0; y < nc; ++y) ptrs.add_target(u->W_targ[y], u->b_targ[y], layers[1 + y]);
    ptrs.add(atk.blob, "the target policy's blob");
    for (int y = 0; y < nc; ++y) ptrs.add(tk[y].blob, "a target critic's blob");
    ptrs.add(ok.blob, "the online actor's blob");
    ptrs.add(u->critic_loss, "critic_loss");
    ptrs.add(u->actor_loss, "actor_loss");
    ptrs.add(u->workspace, "the workspace");
    ptrs.add(u->target, "target");
    ptrs.add(u->q1_next, "q1_next");
    if (nc == 2) ptrs.add(u->q2_next, "q2_next");
    ptrs.add(u->next_action, "next_action");
    if (B > 0) ptrs.add_batch(*u->batch);
    ptrs.add(u->history, "history");
    ptrs.add(u->scale, "scale");                                         // (only read)
    const int hcols = 1 + nc;
    if (int r = ptrs.check(fn, u->history, (size_t)updates * hcols * sizeof(float))) return r;
    if (updates == 0 || B == 0) return 0;
    // ---- the launches' arguments, once
    constexpr size_t fixed = (size_t)BLOCK * (2 * HER_DMAX + 6) * sizeof(float);
    static_assert(fixed + CTR_ACTOR_MAX_BYTES + ACTOR_LDS_SLACK <= LDS_PER_WORKGROUP,
                  "every actor and every critic fit beside the row staging");
    const size_t shm_draw = std::max(atk.bytes, std::max(tk[0].bytes, tk[1].bytes)) + ACTOR_LDS_SLACK;
    size_t shm_critic = 0;
    for (int y = 0; y < nc; ++y)
        shm_critic = std::max(shm_critic, ddpg_critic_fill(gk[y], ap[y], u->batch->obs, u->batch->action, u->scale, u->target, B,
                                                           u->critic_loss ? u->critic_loss + y : nullptr));
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
    ddpg_grad_state(pg, pp);
    pp.loss_scale = -1.0 / (double)B;
    pp.loss = u->actor_loss;
    const TdK td1 = {u->gamma, u->target, u->q1_next, u->next_action};
    const Td3K td2 = {u->gamma, u->sigma, u->clip, u->target, u->q1_next, u->q2_next, u->next_action};
    DdpgTailK ct[2] = {};
    for (int y = 0; y < nc; ++y) ct[y].t = update_tail(ap[y], tk[y], u->W_targ[y], u->b_targ[y], layers[1 + y], u->tau);
    DdpgTailK pt = {update_tail(pp, atk, u->W_targ_actor, u->b_targ_actor, layers[0], u->tau), const_cast<void *>(ok.blob)};
    const unsigned gc = grid_for(std::max(tk[0].bytes, tk[1].bytes) / 16), gp = grid_for(atk.bytes / 16);
    const unsigned ga = grid_for(std::max(ap[0].params, ap[1].params));
    const unsigned slots = (unsigned)ap[0].slots;
    const hipStream_t s = (hipStream_t)stream;
    const HerK hk = {*her};
    // the prefix sums of the stored rows, once: nothing below writes the store
    her_scan(her, tiles, stream);
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
            ct[0].t.hist = hist;
            ct[1].t.hist = hist ? hist + 1 : nullptr;
            pt.t.hist = hist ? hist + nc : nullptr;
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
