// ctr_polyak.inc -- the soft (Polyak) update of the target networks and the refresh of their blobs
// in one launch (ctr_polyak), with its extern "C" entry point.  Included at the end of
// ctr_kernels.hip, after ctr_critic.inc.
//
// Restates the target update of stable-baselines DDPG (ddpg.py get_target_updates: target <-
// (1 - tau) target + tau online, once per training step) as torch.lerp states it, followed by what
// ctr_actor_load / ctr_critic_load do with the result.  The mapping is k_actor_load's (ctr_actor.inc:
// actor_item): one thread per 16 B of a blob owns the eight weights (or four bias floats) that item
// packs, and the fragment layout covers every (row, k) of a layer exactly once, so each target
// element is read and written by one thread only and the update in place needs no ordering.
namespace {

// Kernel-argument copy of one ctr_polyak_net_t: the target's layout and blob, and the tensors.
struct PolyakNetK {
    ActorK ak;
    const float *W[ACTOR_LAYERS], *b[ACTOR_LAYERS];        // online
    float *Wt[ACTOR_LAYERS], *bt[ACTOR_LAYERS];            // target, updated in place
};

struct PolyakK {
    float tau;
    uint32_t end[CTR_POLYAK_MAX_NETS];     // items of nets 0..m (the unused nets: the total)
    PolyakNetK net[CTR_POLYAK_MAX_NETS];
};

// torch's lerp(t, p, tau), every operation rounded to f32 (no fused multiply-add): numpy's float32
// arithmetic, bit for bit.
__device__ __forceinline__ float polyak_lerp(float t, float p, float tau)
{
#pragma clang fp contract(off)
    const float d = p - t;
    if (tau < 0.5f) {
        const float s = tau * d;
        return t + s;
    }
    const float s = d * (1.0f - tau);
    return p - s;
}

__global__ __launch_bounds__(BLOCK) void k_polyak(PolyakK pk)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= pk.end[CTR_POLYAK_MAX_NETS - 1]) return;
    // the item's net, and the item in it; the nets by constant index (they are kernel arguments, and
    // a workgroup may straddle two of them)
    int net = 0;
    uint32_t first = 0;
    #pragma unroll
    for (int m = 0; m + 1 < CTR_POLYAK_MAX_NETS; ++m)
        if (i >= pk.end[m]) {
            net = m + 1;
            first = pk.end[m];
        }
    ActorK ak = pk.net[0].ak;
    #pragma unroll
    for (int m = 1; m < CTR_POLYAK_MAX_NETS; ++m)
        if (net == m) ak = pk.net[m].ak;
    const ActorItem it = actor_item(ak, i - first);
    const float *p = nullptr;
    float *t = nullptr;
    #pragma unroll
    for (int m = 0; m < CTR_POLYAK_MAX_NETS; ++m)
        #pragma unroll
        for (int l = 0; l < ACTOR_LAYERS; ++l)
            if (net == m && it.l == l) {
                p = it.bias ? pk.net[m].b[l] : pk.net[m].W[l];
                t = it.bias ? pk.net[m].bt[l] : pk.net[m].Wt[l];
            }
    float vp[8], v[8];
    actor_item_load(it, p, vp);
    actor_item_load(it, t, v);
    // the new targets, and back to the elements actor_item_load read (the padding stays +0, unstored)
    if (it.bias) {
        #pragma unroll
        for (int j = 0; j < 4; ++j)
            if (it.e + j < it.rows) t[it.e + j] = v[j] = polyak_lerp(v[j], vp[j], pk.tau);
    } else if (it.row < it.rows) {
        float *wr = t + (size_t)it.row * it.cols;
        if (it.l == 0) {
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = actor_k_of(0, it.S, it.h, j);
                if (k < it.cols) wr[k] = v[j] = polyak_lerp(v[j], vp[j], pk.tau);
            }
        } else {
            #pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = polyak_lerp(v[j], vp[j], pk.tau);
            *reinterpret_cast<actor_f32x4u *>(wr + actor_k_of(it.l, it.S, it.h, 0)) = actor_f32x4u{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<actor_f32x4u *>(wr + actor_k_of(it.l, it.S, it.h, 4)) = actor_f32x4u{v[4], v[5], v[6], v[7]};
        }
    }
    static_cast<uint4 *>(const_cast<void *>(ak.blob))[i - first] = actor_item_pack(it, v);
}

int polyak_fail(int net, const char *why)
{
    snprintf(g_err, sizeof g_err, "ctr_polyak: net %d: %s", net, why);
    return CTR_EINVAL;
}

}  // namespace

extern "C" {

int ctr_polyak(const ctr_polyak_net_t *nets, int32_t n_nets, float tau, void *stream)
{
    if (!nets) return fail(CTR_EINVAL, "ctr_polyak: nets is NULL");
    if (n_nets < 1 || n_nets > CTR_POLYAK_MAX_NETS)
        return fail(CTR_EINVAL, "ctr_polyak: n_nets must be in 1..CTR_POLYAK_MAX_NETS (4)");
    PolyakK pk = {};
    uint32_t items = 0;
    for (int m = 0; m < n_nets; ++m) {
        const ctr_polyak_net_t &n = nets[m];
        PolyakNetK &k = pk.net[m];
        if ((n.actor != nullptr) == (n.critic != nullptr))
            return polyak_fail(m, "exactly one of actor and critic must be given");
        if (n.actor ? actor_check(n.actor, &k.ak) : critic_check(n.critic, &k.ak)) {
            char why[sizeof g_err];
            snprintf(why, sizeof why, "%s", g_err);
            snprintf(g_err, sizeof g_err, "ctr_polyak: net %d: %.400s", m, why);
            return CTR_EINVAL;
        }
        if (!n.W || !n.b || !n.W_targ || !n.b_targ) return polyak_fail(m, "W, b, W_targ or b_targ is NULL");
        for (int l = 0; l <= k.ak.n_hidden; ++l) {
            if (!n.W[l] || !n.b[l] || !n.W_targ[l] || !n.b_targ[l])
                return polyak_fail(m, "NULL layer among W, b, W_targ, b_targ [0..n_hidden]");
            if (n.W[l] == n.W_targ[l] || n.b[l] == n.b_targ[l])
                return polyak_fail(m, "an online and a target tensor are the same tensor");
            k.W[l] = n.W[l];
            k.b[l] = n.b[l];
            k.Wt[l] = n.W_targ[l];
            k.bt[l] = n.b_targ[l];
        }
        for (int o = 0; o < m; ++o)
            if (pk.net[o].ak.blob == k.ak.blob) return polyak_fail(m, "shares its blob with an earlier net");
        items += k.ak.bytes / 16;
        pk.end[m] = items;
    }
    for (int m = n_nets; m < CTR_POLYAK_MAX_NETS; ++m) pk.end[m] = items;
    if (!(tau >= 0.f && tau <= 1.f)) return fail(CTR_EINVAL, "ctr_polyak: tau must be in [0, 1]");
    pk.tau = tau;
    hipLaunchKernelGGL(k_polyak, dim3(grid_for(items)), dim3(BLOCK), 0, (hipStream_t)stream, pk);
    return hip_check("ctr_polyak launch");
}

}  // extern "C"
