// ctr_update_common.inc -- what the two update calls share (ctr_sac_update.inc, ctr_ddpg_update.inc):
// the tails' argument struct and tensor selection, and on the host the list of the pointers a call
// touches, the check of a target against its online network and the fill of a tail's arguments.
// Included in ctr_kernels.hip after ctr_sac.inc, before the two.
//
// What the single steps of ctr_ddpg.inc call as well is defined there, before its first caller:
// ddpg_apply_head (element 0's duties: pow, the loss), ddpg_critics_check and ddpg_critic_fill; the
// sampler's two scans are her_scan (ctr_her.inc).  The tails' thread mappings stay in their files.
namespace {

// What a tail takes: the apply launch's arguments, the blob's layout (ak.blob: the blob written),
// the target's tensors (none for SAC's policy) and the history row's entry for this network's loss.
struct UpdateTailK {
    DdpgApplyK ap;
    ActorK ak;
    float *Wt[ACTOR_LAYERS], *bt[ACTOR_LAYERS];
    float tau;
    float *hist;                       // or NULL
};

// An item's tensor: its first flat element among a slot's floats (a bias: bo, its first double among
// the slot's bias sums), and the parameter, gradient, moment and target tensors.
struct UpdateTensors {
    int first, bo;
    float *p, *gp, *mp, *vp, *tp;
};

// The arrays by constant index (they are kernel arguments), per layer, as k_actor_load and k_polyak
// select theirs: a selection by a runtime index (the tensor's 0..7) becomes a table of the pointers
// in scratch.
__device__ __forceinline__ UpdateTensors update_tensors(const UpdateTailK &k, const ActorItem &it)
{
    const DdpgApplyK &a = k.ap;
    UpdateTensors t = {0, a.boff[0], a.p[0], a.g[0], a.m[0], a.v[0], k.Wt[0]};
    #pragma unroll
    for (int l = 0; l < ACTOR_LAYERS; ++l)
        if (it.l == l) {
            t.first = it.bias ? a.end[2 * l] : (l ? a.end[l ? 2 * l - 1 : 0] : 0);
            t.bo = a.boff[l];
            t.p = it.bias ? a.p[2 * l + 1] : a.p[2 * l];
            t.gp = it.bias ? a.g[2 * l + 1] : a.g[2 * l];
            t.mp = it.bias ? a.m[2 * l + 1] : a.m[2 * l];
            t.vp = it.bias ? a.v[2 * l + 1] : a.v[2 * l];
            t.tp = it.bias ? k.bt[l] : k.Wt[l];
        }
    return t;
}

// The base pointers a call writes through or reads, each with its name for the message: nothing the
// call writes may be anything else it touches (as the replaced calls compare them).
struct UpdatePtrs {
    struct Entry {
        const void *p;
        const char *name;
    };
    // the most a call adds: three nets (add_net), three targets (add_target), and the entries added by name,
    // the batch's six among them: 23 in ctr_sac_update, 19 in ctr_ddpg_update
    static constexpr int NAMED = 24, MAX = 3 * (4 * DDPG_TENSORS + 1) + 3 * DDPG_TENSORS + NAMED;
    Entry e[MAX];
    int n = 0;
    bool full = false;                 // an entry nobody counted came: check refuses, nothing is written past e

    void add(const void *p, const char *name)
    {
        if (!p) return;
        if (n == MAX) full = true;
        else e[n++] = Entry{p, name};
    }

    // a learning network's tensors (layers of them) and its pow
    void add_net(const DdpgApplyK &ap, int layers)
    {
        for (int t = 0; t < 2 * layers; ++t) {
            add(ap.p[t], "a parameter tensor");
            add(ap.g[t], "a gradient tensor");
            add(ap.m[t], "a first-moment tensor");
            add(ap.v[t], "a second-moment tensor");
        }
        add(ap.pow, "a net's pow");
    }

    void add_target(float *const *W, float *const *b, int layers)
    {
        for (int l = 0; l < layers; ++l) {
            add(W[l], "a target tensor");
            add(b[l], "a target tensor");
        }
    }

    void add_batch(const ctr_her_batch_t &b)
    {
        add(b.obs, "batch->obs");
        add(b.action, "batch->action");
        add(b.reward, "batch->reward");
        add(b.next_obs, "batch->next_obs");
        add(b.done, "batch->done");
        add(b.index, "batch->index");
    }

    // No two entries are one pointer, and none but history lies inside history's history_bytes.
    int check(const char *fn, const float *history, size_t history_bytes)
    {
        auto same = [&](const char *a, const char *b) {
            snprintf(g_err, sizeof g_err, "%s: %s and %s are the same memory", fn, a, b);
            return CTR_EINVAL;
        };
        if (full) return ddpg_fail(fn, "internal: UpdatePtrs::MAX is too small");
        std::sort(e, e + n, [](const Entry &a, const Entry &b) { return (uintptr_t)a.p < (uintptr_t)b.p; });
        for (int i = 0; i + 1 < n; ++i)
            if (e[i].p == e[i + 1].p) return same(e[i].name, e[i + 1].name);
        if (history) {
            const char *h0 = reinterpret_cast<const char *>(history), *h1 = h0 + history_bytes;
            for (int i = 0; i < n; ++i)
                if (e[i].p != history && (const char *)e[i].p >= h0 && (const char *)e[i].p < h1) return same("history", e[i].name);
        }
        return 0;
    }
};

// A target's layout against its online network's shape.
bool ddpg_same_shape(const ActorK &t, const DdpgNetK &n)
{
    bool same = t.in_dim == n.in_dim && t.n_hidden == n.n_hidden;
    for (int l = 0; same && l < n.n_hidden; ++l) same = 32 * t.tiles[l] == n.width[l];
    return same;
}

// A target against its online network: the shape, then its W / b arrays and their layers 0..n_hidden;
// the three messages are the caller's.
int update_target_check(const char *fn, const ActorK &t, const DdpgNetK &n, float *const *W, float *const *b,
                        const char *shape, const char *arrays, const char *layer)
{
    if (!ddpg_same_shape(t, n)) return ddpg_fail(fn, shape);
    if (!W || !b) return ddpg_fail(fn, arrays);
    for (int l = 0; l <= n.n_hidden; ++l)
        if (!W[l] || !b[l]) return ddpg_fail(fn, layer);
    return 0;
}

// A tail's arguments but hist, which every update sets; W, b: the target's layers, or NULL (no target).
UpdateTailK update_tail(const DdpgApplyK &ap, const ActorK &ak, float *const *W, float *const *b, int layers, float tau)
{
    UpdateTailK k = {};
    k.ap = ap;
    k.ak = ak;
    for (int l = 0; W && l < layers; ++l) {
        k.Wt[l] = W[l];
        k.bt[l] = b[l];
    }
    k.tau = tau;
    return k;
}

}  // namespace
