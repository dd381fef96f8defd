// ctr_her_device.inc -- device side of the HER replay feed (included by ctr_kernels.hip before
// k_step, which records into the store when ctr_step_her is used; the entry points are in
// ctr_her.inc).
namespace {

struct HerK {
    ctr_her_t h;
};

__device__ __forceinline__ int64_t her_slot(const ctr_her_t &h, int64_t e, uint32_t r)
{
    return e * h.slots + (int64_t)(r % (uint32_t)h.slots);
}

// Row addresses are env-minor ([slots][t][n][k]): the lanes of a wave are consecutive envs, which
// mostly sit at the same (slot, t) -- episodes start together and run the same 150 steps -- so a
// wave's record writes are one contiguous span instead of 64 scattered ones.
__device__ __forceinline__ int64_t her_state_row(const ctr_her_t &h, int64_t slot, int t)
{
    const int64_t e = slot / h.slots, s = slot % h.slots;
    return (s * (h.t_max + 1) + t) * h.n + e;
}

__device__ __forceinline__ int64_t her_step_row(const ctr_her_t &h, int64_t slot, int t)
{
    const int64_t e = slot / h.slots, s = slot % h.slots;
    return (s * h.t_max + t) * h.n + e;
}

// One 96-B state row: obs_t in floats 0 .. obs_dim-1 (zero padded to 16), its achieved goal as
// doubles in floats 16 .. 21 -- six dwordx4 stores.
__device__ __forceinline__ void her_put_state(const ctr_her_t &h, int64_t slot, int t, const float *obs,
                                              const double *ag)
{
    float4 *o = reinterpret_cast<float4 *>(h.state + her_state_row(h, slot, t) * 24);
    float v[16];
    #pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = k < 13 ? obs[k] : 0.f;
    if (h.obs_dim == 14) v[13] = obs[13];               // the row has 14 floats only then
    #pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    double2 *a = reinterpret_cast<double2 *>(o + 4);
    a[0] = make_double2(ag[0], ag[1]);
    a[1] = make_double2(ag[2], 0.0);
}

__device__ __forceinline__ const double *her_ag_at(const ctr_her_t &h, int64_t row)
{
    return reinterpret_cast<const double *>(h.state + row * 24 + 16);
}

// Episode r of env e starts: obs_0, its achieved goal, the desired goal (ctr_reach_env.py:114).
__device__ __forceinline__ void her_begin(const ctr_her_t &h, int64_t e, uint32_t r, const float *obs,
                                          const double *ag, const double *dg)
{
    const int64_t s = her_slot(h, e, r);
    h.len[s] = -1;
    h.epoch[s] = r;
    h.dg[3 * s] = dg[0]; h.dg[3 * s + 1] = dg[1]; h.dg[3 * s + 2] = dg[2];
    her_put_state(h, s, 0, obs, ag);
    h.cur_t[e] = 0;
    h.cur_epoch[e] = r;
}

// Every reset of env e opens its next episode, on every path (ctr_her_open after ctr_reset, the
// pooled auto-reset in k_step, the miss sweep, k_her_record): an episode still open is dropped.
__device__ __forceinline__ void her_reopen(const ctr_her_t &h, int64_t e, uint32_t r, const float *obs,
                                           const double *ag, const double *dg)
{
    if (h.cur_t[e] >= 0) h.len[her_slot(h, e, h.cur_epoch[e])] = 0;   // unfinished episode: dropped
    her_begin(h, e, r, obs, ag, dg);
}

__global__ __launch_bounds__(BLOCK) void k_her_open(HerK hk, ctr_batch_t b, const float *__restrict__ obs,
                                                    const uint8_t *__restrict__ mask)
{
    const ctr_her_t &h = hk.h;
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= h.n || (mask && !mask[e])) return;
    her_reopen(h, e, b.epoch[e], obs + h.obs_dim * e, b.achieved_goal + 3 * e, b.desired_goal + 3 * e);
}

// HindsightExperienceReplayWrapper.add(obs_t, action, reward, obs_tp1, done) for env e: the
// transition goes into the env's open episode; on done (or at t_max) the episode is stored
// (len = L, sampleable from then on).  obs_t1 / ag_t1 are the step's observation and achieved
// goal before any auto-reset (the terminal ones of a done env).  Returns true when the episode
// was closed; the caller opens the env's next episode (her_begin) once it is reset.
__device__ __forceinline__ bool her_record_lane(const ctr_her_t &h, int64_t e, const float *a, float reward,
                                                bool done, const float *obs_t1, const double *ag_t1, double tol)
{
    const int t = h.cur_t[e];
    if (t < 0) return false;                             // no open episode (done without auto-reset)
    const int64_t s = her_slot(h, e, h.cur_epoch[e]);
    float4 *st = reinterpret_cast<float4 *>(h.step + her_step_row(h, s, t) * 8);
    st[0] = make_float4(a[0], a[1], a[2], a[3]);
    st[1] = make_float4(a[4], a[5], reward, 0.f);
    her_put_state(h, s, t + 1, obs_t1, ag_t1);
    if (done || t + 1 >= h.t_max) {
        h.tol[s] = tol;
        h.len[s] = t + 1;
        h.cur_t[e] = -1;
        return true;
    }
    h.cur_t[e] = t + 1;
    return false;
}

// Records the step ctr_step just made, from its outputs (the unfused path; ctr_step_her records
// inside k_step instead).
__global__ __launch_bounds__(BLOCK) void k_her_record(HerK hk, ctr_batch_t b, const float *__restrict__ actions,
                                                      ctr_step_out_t o, double tol)
{
    const ctr_her_t &h = hk.h;
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= h.n) return;
    const bool done = o.done[e] != 0;
    const float *obs = static_cast<const float *>(o.obs);           // HER runs on float32 observations
    const float *tobs = static_cast<const float *>(o.terminal_obs);
    her_record_lane(h, e, actions + 6 * e, o.reward[e], done,
                    done ? tobs + h.obs_dim * e : obs + h.obs_dim * e,
                    done ? o.terminal_achieved + 3 * e : b.achieved_goal + 3 * e, tol);
    if (done && b.t[e] == 0)                             // auto-reset: the next episode starts now
        her_reopen(h, e, b.epoch[e], obs + h.obs_dim * e, b.achieved_goal + 3 * e, b.desired_goal + 3 * e);
}

__device__ __forceinline__ int64_t her_rows(const ctr_her_t &h, int64_t L)
{
    // _store_episode: every transition is stored; FUTURE adds k relabels to all but the last
    return h.strategy == CTR_HER_FUTURE ? L + (int64_t)h.n_sampled_goal * (L - 1) : L * (1 + h.n_sampled_goal);
}

// _sample_achieved_goal for row j >= 1 of transition t of an L-transition episode: the index sel
// of the transition whose obs_t supplies the goal (a pure function of the episode and (t, j)).
__device__ __forceinline__ int her_sel(const ctr_her_t &h, int64_t genv, uint32_t epoch, int t, int j, int L)
{
    if (h.strategy == CTR_HER_FINAL) return L - 1;
    uint32_t c[4] = {(uint32_t)t | ((uint32_t)j << 16), epoch, (uint32_t)genv,
                     (uint32_t)((uint64_t)genv >> 32) ^ (4u << 24)};
    philox(c, (uint32_t)h.seed, (uint32_t)(h.seed >> 32));
    const double u = u53(c[0], c[1]);
    const int lo = h.strategy == CTR_HER_FUTURE ? t + 1 : 0;   // np.arange(lo, L)
    int sel = lo + (int)(u * (double)(L - lo));
    return sel < L ? sel : L - 1;
}

// np.linalg.norm(ag - dg, axis=-1): unfused squares and sums, as numpy evaluates them
__device__ __forceinline__ double her_dist(const double *a, const double *g)
{
#pragma clang fp contract(off)
    const double dx = a[0] - g[0], dy = a[1] - g[1], dz = a[2] - g[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// A 96-B state row as six 16-B loads: obs in v[0..15], the achieved goal in ag[0..2].
struct StateRow {
    float v[16];
    double ag[3];
};

__device__ __forceinline__ StateRow her_load_state(const ctr_her_t &h, int64_t row)
{
    const float4 *p = reinterpret_cast<const float4 *>(h.state + row * 24);
    StateRow sr;
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 x = p[q];
        sr.v[4 * q] = x.x; sr.v[4 * q + 1] = x.y; sr.v[4 * q + 2] = x.z; sr.v[4 * q + 3] = x.w;
    }
    const double2 a0 = reinterpret_cast<const double2 *>(p + 4)[0], a1 = reinterpret_cast<const double2 *>(p + 4)[1];
    sr.ag[0] = a0.x; sr.ag[1] = a0.y; sr.ag[2] = a1.x;
    return sr;
}

// HERGoalEnvWrapper.convert_dict_to_obs of a loaded state row (static indices only, so the row
// stays in registers): [observation, achieved_goal, desired_goal].
__device__ __forceinline__ void her_put_row(float *dst, const StateRow &sr, bool has14, const double *goal)
{
    #pragma unroll
    for (int k = 0; k < 13; ++k) dst[k] = sr.v[k];
    if (has14) dst[13] = sr.v[13];
    float *g = dst + (has14 ? 14 : 13);
    #pragma unroll
    for (int k = 0; k < 3; ++k) { g[k] = (float)sr.ag[k]; g[3 + k] = (float)goal[k]; }
}

// The block's rows are staged in LDS and written out as one contiguous span per array (whole
// 16-B stores) instead of 19-float rows scattered lane by lane.
__device__ __forceinline__ void her_flush(float *__restrict__ dst, const float *__restrict__ src, int64_t count)
{
    // dst is 16-B aligned: the block's first row starts at a multiple of BLOCK rows of d floats
    const int64_t n4 = count / 4;
    for (int64_t k = threadIdx.x; k < n4; k += BLOCK)
        reinterpret_cast<float4 *>(dst)[k] = reinterpret_cast<const float4 *>(src)[k];
    for (int64_t k = 4 * n4 + threadIdx.x; k < count; k += BLOCK) dst[k] = src[k];
}

// ---- the sampler's prefix sums: rows stored per slot -> CDF over slots (two launches) ----
constexpr int HER_TILE = CTR_HER_SCAN_TILE;              // slots per scan tile, 4 per lane
static_assert(HER_TILE == 4 * BLOCK, "a scan tile is 4 slots per lane");

__device__ __forceinline__ int64_t her_slot_rows(const ctr_her_t &h, int64_t s)
{
    const int len = h.len[s];
    return len > 0 ? her_rows(h, len) : 0;
}

// Inclusive scan of one value per lane over the workgroup: wave64 shuffles, then the 4 wave
// totals through LDS.  Every lane of the workgroup must call it.
__device__ __forceinline__ int64_t her_block_scan(int64_t v, int64_t &total)
{
    __shared__ int64_t s_w[BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t x = __shfl_up(v, o);
        v += lane >= o ? x : 0;
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    int64_t off = 0;
    total = 0;
    #pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) {
        off += k < w ? s_w[k] : 0;
        total += s_w[k];
    }
    __syncthreads();
    return v + off;
}

// Pass 1: cdf[s] = rows stored in slots tile_start .. s (tile-local inclusive sums);
// cdf[E + tile] = the tile's total.
__global__ __launch_bounds__(BLOCK) void k_her_scan_tiles(HerK hk)
{
    const ctr_her_t &h = hk.h;
    const int64_t E = h.n * h.slots;
    const int64_t s0 = (int64_t)blockIdx.x * HER_TILE + 4 * threadIdx.x;
    int64_t r[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = s0 + k < E ? her_slot_rows(h, s0 + k) : 0;
    const int64_t mine = (r[0] + r[1]) + (r[2] + r[3]);
    int64_t total;
    int64_t acc = her_block_scan(mine, total) - mine;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc += r[k];
        if (s0 + k < E) h.cdf[s0 + k] = acc;
    }
    if (threadIdx.x == 0) h.cdf[E + blockIdx.x] = total;
}

// Pass 2 (one workgroup): tile totals -> exclusive tile offsets in place; the stored-row count
// after them, at cdf[E + tiles].
__global__ __launch_bounds__(BLOCK) void k_her_scan_tops(HerK hk, int64_t tiles)
{
    const ctr_her_t &h = hk.h;
    int64_t *top = h.cdf + h.n * h.slots;
    int64_t carry = 0;
    for (int64_t base = 0; base < tiles; base += BLOCK) {       // uniform trip count
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < tiles ? top[i] : 0;
        int64_t total;
        const int64_t incl = her_block_scan(v, total);
        if (i < tiles) top[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) top[tiles] = carry;
}

// ReplayBuffer.sample(batch_size): rows uniformly with replacement over the stored rows.  Row u
// (one uniform integer below the stored-row count) is found by inverse CDF: the tile whose
// offset range holds u, then the slot inside the tile, by binary search over the prefix sums.
//
// her_sample_row: the row of this lane (row blockIdx.x * BLOCK + threadIdx.x of the batch), formed
// into the block's LDS staging (s_obs / s_nobs [BLOCK][d], s_act [BLOCK][6]; a zero row when nothing
// is stored or the lane is past B), its reward, done and index stored; rew and dn return the two
// stored values.  Both samplers (k_her_sample, k_her_sample_td) call it, then a barrier, then
// her_flush_batch.
constexpr int HER_DMAX = 20;                              // obs_dim + 6 <= 20

__device__ __forceinline__ void her_sample_row(const ctr_her_t &h, int64_t B, uint64_t seed, uint64_t counter,
                                               const ctr_her_batch_t &out, float *s_obs, float *s_nobs, float *s_act,
                                               float &rew, float &dn)
{
    const int64_t i0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t i = i0 + threadIdx.x;
    const bool live = i < B;
    const int64_t E = h.n * h.slots;
    const int64_t tiles = (E + HER_TILE - 1) / HER_TILE;
    const int64_t *top = h.cdf + E;
    const int64_t stored = top[tiles];
    const int d = h.obs_dim + 6;
    int64_t slot = -1, r = 0;
    int L = 0;
    if (live && stored > 0) {
        uint32_t c[4] = {0u, (uint32_t)counter, (uint32_t)i, (uint32_t)(counter >> 32) ^ (5u << 24)};
        philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        int64_t u = (int64_t)(u53(c[0], c[1]) * (double)stored);
        u = u < stored ? u : stored - 1;
        // the last tile whose offset is <= u (an empty tile shares its offset with the next one)
        int64_t lo = 0, hi = tiles - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (top[mid] <= u) lo = mid;
            else hi = mid - 1;
        }
        const int64_t v = u - top[lo];
        // the first slot of the tile whose inclusive count exceeds v (empty slots never do)
        const int64_t first = lo * HER_TILE;
        int64_t a = first, b = (first + HER_TILE < E ? first + HER_TILE : E) - 1;
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (h.cdf[mid] > v) b = mid;
            else a = mid + 1;
        }
        slot = a;
        r = v - (a > first ? h.cdf[a - 1] : 0);
        L = h.len[slot];
    }
    float *so = s_obs + threadIdx.x * d, *sn = s_nobs + threadIdx.x * d, *sa = s_act + threadIdx.x * 6;
    int t = 0, j = 0;
    rew = 0.f;
    dn = 0.f;
    if (slot < 0) {                                       // nothing stored (yet), or past B: zero row
        for (int k = 0; k < d; ++k) { so[k] = 0.f; sn[k] = 0.f; }
        for (int k = 0; k < 6; ++k) sa[k] = 0.f;
    } else {
        const int per = 1 + h.n_sampled_goal;
        t = (int)(r / per);
        j = (int)(r % per);                               // _store_episode order: real row, then k relabels
        const int64_t row_t = her_state_row(h, slot, t), row_n = row_t + h.n;
        const StateRow st = her_load_state(h, row_t), sx = her_load_state(h, row_n);
        const float4 *stp = reinterpret_cast<const float4 *>(h.step + her_step_row(h, slot, t) * 8);
        const float4 s0 = stp[0], s1 = stp[1];
        double goal[3] = {h.dg[3 * slot], h.dg[3 * slot + 1], h.dg[3 * slot + 2]};
        rew = s1.z;
        dn = (t == L - 1) ? 1.f : 0.f;
        if (j > 0) {
            const int64_t genv = h.env_base + slot / h.slots;
            const int sel = her_sel(h, genv, h.epoch[slot], t, j, L);
            const double *g = her_ag_at(h, her_state_row(h, slot, sel));
            goal[0] = g[0]; goal[1] = g[1]; goal[2] = g[2];
            rew = (her_dist(sx.ag, goal) > h.tol[slot]) ? -1.0f : 0.0f;   // compute_reward, ctr_reach_env.py:170
            dn = 0.f;
        }
        her_put_row(so, st, h.obs_dim == 14, goal);
        her_put_row(sn, sx, h.obs_dim == 14, goal);
        sa[0] = s0.x; sa[1] = s0.y; sa[2] = s0.z; sa[3] = s0.w; sa[4] = s1.x; sa[5] = s1.y;
    }
    if (live) {
        out.reward[i] = rew;
        out.done[i] = dn;
        if (out.index) {
            out.index[3 * i] = (int32_t)slot;
            out.index[3 * i + 1] = slot < 0 ? 0 : t;
            out.index[3 * i + 2] = slot < 0 ? 0 : j;
        }
    }
}

// The block's staged rows to out.obs / out.next_obs / out.action (after a barrier behind her_sample_row).
__device__ __forceinline__ void her_flush_batch(const ctr_her_t &h, int64_t B, const ctr_her_batch_t &out,
                                                const float *s_obs, const float *s_nobs, const float *s_act)
{
    const int64_t i0 = (int64_t)blockIdx.x * BLOCK;
    const int d = h.obs_dim + 6;
    const int64_t cnt = (B - i0) < BLOCK ? (B - i0) : BLOCK;
    her_flush(out.obs + i0 * d, s_obs, cnt * d);
    her_flush(out.next_obs + i0 * d, s_nobs, cnt * d);
    her_flush(out.action + i0 * 6, s_act, cnt * 6);
}

__global__ __launch_bounds__(BLOCK) void k_her_sample(HerK hk, int64_t B, uint64_t seed, uint64_t counter,
                                                      ctr_her_batch_t out)
{
    __shared__ __attribute__((aligned(16))) float s_obs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_nobs[BLOCK * HER_DMAX];
    __shared__ __attribute__((aligned(16))) float s_act[BLOCK * 6];
    float rew, dn;
    her_sample_row(hk.h, B, seed, counter, out, s_obs, s_nobs, s_act, rew, dn);
    __syncthreads();
    her_flush_batch(hk.h, B, out, s_obs, s_nobs, s_act);
}

}  // namespace
