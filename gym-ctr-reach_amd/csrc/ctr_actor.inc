// ctr_actor.inc -- the deterministic MLP actor (ctr_actor, and the actor of k_rollout): its
// arithmetic, the packed weight blob and its packers, on the host (mlp_pack) and on the device
// (k_actor_load).  Included by ctr_kernels.hip inside its anonymous namespace.  The MLP critic
// (ctr_critic.inc) is the same code with another shape: a row of 25 or 26 floats [row, action]
// (actor_tile<26>) and a one-row output layer without tanh (ActorK::out_rows = 1); layout, packers
// and the column-tile function are shared, not copied.
//
// The network (include/ctr_reach_amd.h, "MLP actor"): 1..3 hidden layers of width 32..256 (multiples
// of 32) on the flat row x[in_dim] = [observation, achieved_goal, desired_goal], zero-padded to 32:
//     x_hi = bf16(x);  x_lo = bf16(x - float(x_hi))
//     h1   = bf16(relu(W1 x_hi + W1 x_lo + b1))        bf16 weights, f32 accumulation, f32 bias
//     hl   = bf16(relu(Wl h(l-1) + bl))
//     y    = Wout hL + bout ;  a_i = scale_i * tanhf(y_i)
// relu(z) = z > 0 ? z : 0 (a NaN becomes 0); every bf16 rounding is to nearest even.
//
// Mapping: v_mfma_f32_32x32x16_bf16 with the weights as the A operand and the activations as the B
// operand, whose 32 columns are 32 envs: a wave's 64 envs are two column tiles.  A layer's f32
// result tile has its env on the lane and 16 of its features in the lane's registers, and the next
// layer sums over features, so the tile, converted to bf16, IS the next layer's B fragment: no lane
// movement and no LDS between the layers.  Register 8s + j of lane half h is feature
// 16s + 8(j>>2) + 4h + (j&3) of the tile, so k-step s of the next layer runs over the tile's features
// in that order, and the packer stores the weight fragments of every layer but the first in the same
// order (actor_k_of: the only place that knows the permutation).  Lanes move twice: the input rows
// (lane l owns env l; the first layer's fragment wants k = 8h + j of env 32c + (l & 31)) and the six
// outputs (rows 0..3 on lane half 0, 4..5 on half 1), both by wave-local lane permutes.  Nothing in
// the actor waits for another wave; an output column depends on its own input column only.
//
// Blob: per layer, per 32-row tile T, per k-step S, the 64 lanes' 8-element bf16 fragments (16 B
// each, lane-major: one 1-KB ds_read_b128 sweep per MFMA); then the f32 biases of every layer, each
// padded to whole 32-row tiles.

typedef __bf16 actor_bf16x8 __attribute__((ext_vector_type(8)));
typedef float actor_f32x16 __attribute__((ext_vector_type(16)));

constexpr int ACTOR_LAYERS = CTR_ACTOR_MAX_HIDDEN + 1;         // the hidden layers and the output layer
constexpr int ACTOR_TILES = CTR_ACTOR_MAX_WIDTH / 32;          // 32-row tiles of the widest layer

// Kernel-argument copy of the actor, with the blob's layout.
struct ActorK {
    int32_t in_dim, n_hidden;
    int32_t tiles[ACTOR_LAYERS];       // 32-row tiles of layer l's output (0 past the output layer)
    uint32_t w_off[ACTOR_LAYERS];      // byte offset of layer l's fragments
    uint32_t b_off[ACTOR_LAYERS];      // byte offset of layer l's biases
    uint32_t bytes;                    // whole blob
    float scale[6];                    // the actor's action box (the critic has none: zeros)
    int32_t out_rows;                  // rows of the output layer: 6 (the actor), 1 (the critic); in what
                                       // was padding, so the period kernels' arguments stay where they were
    const void *blob;
};

// k index of element j of lane half h in k-step S of layer l (see the header comment).
__host__ __device__ inline int actor_k_of(int l, int S, int h, int j)
{
    if (l == 0) return 16 * S + 8 * h + j;
    return 32 * (S >> 1) + 16 * (S & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
}

// float -> bf16 bits in integer arithmetic (host and device: k_actor_load gives the host packer's bits)
__host__ __device__ inline uint16_t actor_bf16_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);     // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                      // nearest even
}

// An MLP's shape as its public struct gives it (ctr_actor_t, ctr_critic_t): what the two networks
// differ in is the input row and the rows of the output layer.
struct MlpShape {
    const char *who;                   // "actor" / "critic", in the messages
    int in_extra;                      // in_dim = obs_dim + in_extra (obs_dim 13 or 14)
    int out_rows;
    int32_t in_dim, n_hidden;
    const int32_t *width;
};

// The shape checks of every actor and critic entry point; fills the layout.
int mlp_layout(const MlpShape &m, ActorK *ak)
{
    if (m.in_dim != 13 + m.in_extra && m.in_dim != 14 + m.in_extra) {
        snprintf(g_err, sizeof g_err, "%s: in_dim must be obs_dim + %d = %d or %d", m.who, m.in_extra, 13 + m.in_extra,
                 14 + m.in_extra);
        return CTR_EINVAL;
    }
    if (m.n_hidden < 1 || m.n_hidden > CTR_ACTOR_MAX_HIDDEN) {
        snprintf(g_err, sizeof g_err, "%s: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)", m.who);
        return CTR_EINVAL;
    }
    for (int l = 0; l < m.n_hidden; ++l)
        if (m.width[l] < 32 || m.width[l] > CTR_ACTOR_MAX_WIDTH || m.width[l] % 32) {
            snprintf(g_err, sizeof g_err, "%s: every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)",
                     m.who);
            return CTR_EINVAL;
        }
    memset(ak, 0, sizeof *ak);
    ak->in_dim = m.in_dim;
    ak->n_hidden = m.n_hidden;
    ak->out_rows = m.out_rows;
    int64_t off = 0, wbytes = 0;
    for (int l = 0; l <= m.n_hidden; ++l) {
        const int tiles = l < m.n_hidden ? m.width[l] / 32 : 1;
        const int ksteps = l == 0 ? 2 : m.width[l - 1] / 16;
        ak->tiles[l] = tiles;
        ak->w_off[l] = (uint32_t)off;
        off += (int64_t)tiles * ksteps * 1024;
    }
    wbytes = off;
    for (int l = 0; l <= m.n_hidden; ++l) {
        ak->b_off[l] = (uint32_t)off;
        off += (int64_t)ak->tiles[l] * 32 * 4;
    }
    if (off > CTR_ACTOR_MAX_BYTES) {
        snprintf(g_err, sizeof g_err, "%s: the packed network (%lld B of weights + %lld B of biases) exceeds "
                 "CTR_ACTOR_MAX_BYTES = %d B of LDS", m.who, (long long)wbytes, (long long)(off - wbytes), CTR_ACTOR_MAX_BYTES);
        return CTR_EINVAL;
    }
    ak->bytes = (uint32_t)off;
    return 0;
}

int actor_layout(const ctr_actor_t *a, ActorK *ak)
{
    if (!a) return fail(CTR_EINVAL, "actor is NULL");
    return mlp_layout(MlpShape{"actor", 6, 6, a->in_dim, a->n_hidden, a->width}, ak);
}

int critic_layout(const ctr_critic_t *c, ActorK *ak)
{
    if (!c) return fail(CTR_EINVAL, "critic is NULL");
    return mlp_layout(MlpShape{"critic", 12, 1, c->in_dim, c->n_hidden, c->width}, ak);
}

// The blob pointer of the entry points that read or write it.
int mlp_blob(const char *who, const void *blob, ActorK *ak)
{
    if (!blob) {
        snprintf(g_err, sizeof g_err, "%s: blob is NULL", who);
        return CTR_EINVAL;
    }
    if (((uintptr_t)blob & 15u) != 0) {
        snprintf(g_err, sizeof g_err, "%s: blob must be 16-B aligned", who);
        return CTR_EINVAL;
    }
    ak->blob = blob;
    return 0;
}

// ... and the checks of the entry points that run it.
int actor_check(const ctr_actor_t *a, ActorK *ak)
{
    if (int r = actor_layout(a, ak)) return r;
    for (int i = 0; i < 6; ++i) {
        if (!isfinite(a->scale[i])) return fail(CTR_EINVAL, "actor: scale must be finite");
        ak->scale[i] = a->scale[i];
    }
    return mlp_blob("actor", a->blob, ak);
}

int critic_check(const ctr_critic_t *c, ActorK *ak)
{
    if (int r = critic_layout(c, ak)) return r;
    return mlp_blob("critic", c->blob, ak);
}

// The host packer of both networks (ctr_actor_pack, ctr_critic_pack: `fn`): the shape is ak's.
int mlp_pack(const ActorK &ak, const char *fn, const float *const *W, const float *const *b, void *blob_host)
{
    if (!W || !b || !blob_host) {
        snprintf(g_err, sizeof g_err, "%s: NULL argument", fn);
        return CTR_EINVAL;
    }
    for (int l = 0; l <= ak.n_hidden; ++l)
        if (!W[l] || !b[l]) {
            snprintf(g_err, sizeof g_err, "%s: NULL layer among W[0..n_hidden], b[0..n_hidden]", fn);
            return CTR_EINVAL;
        }
    char *out = static_cast<char *>(blob_host);
    memset(out, 0, ak.bytes);
    for (int l = 0; l <= ak.n_hidden; ++l) {
        const int rows = l < ak.n_hidden ? 32 * ak.tiles[l] : ak.out_rows;
        const int cols = l == 0 ? ak.in_dim : 32 * ak.tiles[l - 1];
        const int ksteps = l == 0 ? 2 : cols / 16;
        for (int T = 0; T < ak.tiles[l]; ++T)
            for (int S = 0; S < ksteps; ++S)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int row = 32 * T + (lane & 31), k = actor_k_of(l, S, lane >> 5, j);
                        const uint16_t v = (row < rows && k < cols) ? actor_bf16_bits(W[l][(size_t)row * cols + k]) : 0;
                        memcpy(out + ak.w_off[l] + ((size_t)(T * ksteps + S) * 64 + lane) * 16 + 2 * j, &v, 2);
                    }
        memcpy(out + ak.b_off[l], b[l], (size_t)rows * 4);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// The packer on the device (ctr_actor_load, ctr_critic_load): mlp_pack's bytes from device-resident
// parameters, so that a trainer refreshes the blob after an optimiser step without a copy to the host.  One thread
// per 16 B of the blob: a weight fragment (lane `lane` of k-step S of tile T of layer l) or four
// bias floats.  Every byte of the blob is written, the padding as zero; no thread reads what another
// wrote.
struct ActorSrc {
    const float *W[ACTOR_LAYERS];      // device, row-major [out][in]
    const float *b[ACTOR_LAYERS];      // device, [out]
};

typedef float actor_f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a parameter tensor may start at any float

// Item i (16 B) of a blob and the elements of its layer's parameter tensors that it holds: the one
// place that knows the packer's thread-to-element mapping on the device (k_actor_load, and k_polyak
// in ctr_polyak.inc, which also writes those elements).  A bias item holds b[e .. e + 3] below
// rows; a weight item holds, of row `row` (when below rows), the columns actor_k_of(l, S, h, 0..7)
// below cols.
struct ActorItem {
    bool bias;
    int l, rows, cols;                 // the layer, and its real rows and columns
    int e;                             // bias: the first of its four floats
    int row, S, h;                     // weights: the fragment's row, k-step and lane half
};

__device__ __forceinline__ ActorItem actor_item(const ActorK &ak, uint32_t i)
{
    ActorItem it = {};
    const uint32_t byte = 16 * i;
    it.bias = byte >= ak.b_off[0];
    // the item's layer and its place in it; the arrays by constant index (they are kernel arguments)
    uint32_t off = 0;
    #pragma unroll
    for (int m = 0; m < ACTOR_LAYERS; ++m) {
        const uint32_t start = it.bias ? ak.b_off[m] : ak.w_off[m];
        if (m <= ak.n_hidden && byte >= start) {
            it.l = m;
            off = byte - start;
            it.rows = m < ak.n_hidden ? 32 * ak.tiles[m] : ak.out_rows;
            it.cols = m == 0 ? ak.in_dim : 32 * ak.tiles[m - 1];
        }
    }
    if (it.bias) {
        it.e = (int)(off / 4);
    } else {
        const int ksteps = it.l == 0 ? 2 : it.cols / 16;
        const int f = (int)(off / 16), lane = f & 63, ts = f >> 6;
        const int T = ts / ksteps;
        it.h = lane >> 5;
        it.S = ts - T * ksteps;
        it.row = 32 * T + (lane & 31);
    }
    return it;
}

// The item's elements of one layer's tensors (p = b for a bias item, W for a weight item) as bits in
// flight: v[0..3] the bias floats, v[0..7] the fragment's weights; what lies past the tensor is +0
// and is not read.
__device__ __forceinline__ void actor_item_load(const ActorItem &it, const float *p, float v[8])
{
    #pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (it.bias) {
        // rows is 6 or 1 in the output layer, so the tail is guarded per float
        #pragma unroll
        for (int t = 0; t < 4; ++t)
            if (it.e + t < it.rows) v[t] = p[it.e + t];
    } else if (it.row < it.rows) {
        const float *wr = p + (size_t)it.row * it.cols;
        if (it.l == 0) {
            // eight consecutive floats of an in_dim-float row (19 or 20; the critic's: 25 or 26)
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = actor_k_of(0, it.S, it.h, j);
                if (k < it.cols) v[j] = wr[k];
            }
        } else {
            // two runs of four (cols is a multiple of 32, so both lie inside the row)
            const actor_f32x4u a0 = *reinterpret_cast<const actor_f32x4u *>(wr + actor_k_of(it.l, it.S, it.h, 0));
            const actor_f32x4u a1 = *reinterpret_cast<const actor_f32x4u *>(wr + actor_k_of(it.l, it.S, it.h, 4));
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = a0[j];
                v[4 + j] = a1[j];
            }
        }
    }
}

// The item's 16 B of the blob from those elements: the biases copied as bits, the weights rounded.
__device__ __forceinline__ uint4 actor_item_pack(const ActorItem &it, const float v[8])
{
    uint32_t w[4];
    #pragma unroll
    for (int j = 0; j < 4; ++j)
        w[j] = it.bias ? __float_as_uint(v[j])
                       : (uint32_t)actor_bf16_bits(v[2 * j]) | ((uint32_t)actor_bf16_bits(v[2 * j + 1]) << 16);   // +0 -> 0
    return uint4{w[0], w[1], w[2], w[3]};
}

__global__ __launch_bounds__(BLOCK) void k_actor_load(ActorK ak, ActorSrc src, void *__restrict__ blob)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ak.bytes / 16) return;
    const ActorItem it = actor_item(ak, i);
    const float *p = nullptr;
    #pragma unroll
    for (int m = 0; m < ACTOR_LAYERS; ++m)
        if (m == it.l) p = it.bias ? src.b[m] : src.W[m];
    float v[8];
    actor_item_load(it, p, v);
    static_cast<uint4 *>(blob)[i] = actor_item_pack(it, v);
}

// The launch of ctr_actor_load / ctr_critic_load (`fn`), after the shape checks: ak.blob not yet set.
int mlp_load(ActorK &ak, const char *who, const char *fn, const void *blob, const float *const *W,
             const float *const *b, void *stream)
{
    if (!W || !b) {
        snprintf(g_err, sizeof g_err, "%s: W or b is NULL", fn);
        return CTR_EINVAL;
    }
    ActorSrc src = {};
    for (int l = 0; l <= ak.n_hidden; ++l) {
        if (!W[l] || !b[l]) {
            snprintf(g_err, sizeof g_err, "%s: NULL layer among W[0..n_hidden], b[0..n_hidden]", fn);
            return CTR_EINVAL;
        }
        src.W[l] = W[l];
        src.b[l] = b[l];
    }
    if (int r = mlp_blob(who, blob, &ak)) return r;
    hipLaunchKernelGGL(k_actor_load, dim3(grid_for(ak.bytes / 16)), dim3(BLOCK), 0, (hipStream_t)stream, ak, src,
                       const_cast<void *>(blob));
    char what[64];
    snprintf(what, sizeof what, "%s launch", fn);
    return hip_check(what);
}

// ------------------------------------------------------------------------------------------
// Device side.  The blob sits in dynamic LDS behind the per-lane domain tables (lane_bytes of
// them), at the next 16-B boundary (the static LDS in front of the dynamic region need not be a
// multiple of 16; a misaligned ds_read_b128 is replayed): launch with ACTOR_LDS_SLACK more.
constexpr size_t ACTOR_LDS_SLACK = 16;

__device__ __forceinline__ char *actor_lds_base(size_t lane_bytes)
{
    char *p = reinterpret_cast<char *>(s_lane_dyn) + lane_bytes;
    const uint32_t a = (uint32_t)(size_t)(__attribute__((address_space(3))) char *)p;
    return p + ((0u - a) & 15u);
}

// Every lane of the workgroup: the blob from global memory into LDS (a barrier must follow).
__device__ __forceinline__ void actor_stage(const ActorK &ak, char *lds)
{
    const uint4 *src = static_cast<const uint4 *>(ak.blob);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (uint32_t i = threadIdx.x; i < ak.bytes / 16; i += BLOCK) dst[i] = src[i];
}

__device__ __forceinline__ actor_bf16x8 actor_frag(const char *w, int index, int lane)
{
    return *reinterpret_cast<const actor_bf16x8 *>(w + (size_t)index * 1024 + lane * 16);
}

// The flat row of an env from its observation (already rounded to f32), achieved and desired goal.
__device__ __forceinline__ void actor_row(const float ob[14], const float ag[3], const float dg[3], bool multi,
                                          float x[20])
{
    #pragma unroll
    for (int k = 0; k < 13; ++k) x[k] = ob[k];
    x[13] = multi ? ob[13] : ag[0];
    x[14] = multi ? ag[0] : ag[1];
    x[15] = multi ? ag[1] : ag[2];
    x[16] = multi ? ag[2] : dg[0];
    x[17] = multi ? dg[0] : dg[1];
    x[18] = multi ? dg[1] : dg[2];
    x[19] = multi ? dg[2] : 0.f;
}

// bias, relu, bf16: the f32 tile T of a layer becomes k-steps 2T, 2T + 1 of the next one
__device__ __forceinline__ void actor_activate(const actor_f32x16 &acc, const float *bias, int T, int h,
                                               actor_bf16x8 &f0, actor_bf16x8 &f1)
{
    float z[16];
    #pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 bb = *reinterpret_cast<const float4 *>(bias + 32 * T + 8 * g + 4 * h);
        z[4 * g] = acc[4 * g] + bb.x;
        z[4 * g + 1] = acc[4 * g + 1] + bb.y;
        z[4 * g + 2] = acc[4 * g + 2] + bb.z;
        z[4 * g + 3] = acc[4 * g + 3] + bb.w;
    }
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        f0[j] = (__bf16)(z[j] > 0.f ? z[j] : 0.f);
        f1[j] = (__bf16)(z[8 + j] > 0.f ? z[8 + j] : 0.f);
    }
}


// One 32-env column tile c of the wave through the network, up to the output layer's f32 tile with
// its bias added (rows 0..3 of env 32c + r on lane r, rows 4..7 on lane 32 + r, in acc[0..3]).
// Every lane of the wave calls it (wave-uniform control flow): x = this lane's env's row of NX
// floats (NX = 20, the actor's: x[19] = 0 when in_dim is 19; NX = 26, the critic's: x[25] = 0 when
// in_dim is 25), zero-padded to 32 here; lds = the staged blob.
template <int NX>
__device__ __forceinline__ actor_f32x16 actor_tile(const ActorK &ak, const char *lds, const float *x, int c)
{
    static_assert(NX > 16 && NX <= 32, "two k-steps over 32 padded inputs");
    const int lane = (int)(threadIdx.x & 63), h = lane >> 5, r = lane & 31;
    const actor_f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const actor_bf16x8 fzero = {0, 0, 0, 0, 0, 0, 0, 0};
    // the input fragments of column tile c: k-step 0 = features 8h + j, k-step 1 = features
    // 16 + 8h + j (those below NX exist: lane half 1 has none for the actor), each split into
    // bf16 hi + lo
    const int src = 32 * c + r;
    actor_bf16x8 xh[2], xl[2];
    xh[1] = fzero;
    xl[1] = fzero;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v0 = __shfl(x[j], src), v1 = __shfl(x[8 + j], src);
        const float v = h ? v1 : v0;
        const __bf16 hi = (__bf16)v;
        xh[0][j] = hi;
        xl[0][j] = (__bf16)(v - (float)hi);
    }
    #pragma unroll
    for (int j = 0; j < (NX - 16 < 8 ? NX - 16 : 8); ++j) {
        const float v1 = __shfl(x[16 + j], src);
        float v = h ? 0.f : v1;
        if (24 + j < NX) {
            const float v2 = __shfl(x[24 + j < NX ? 24 + j : 0], src);
            v = h ? v2 : v1;
        }
        const __bf16 hi = (__bf16)v;
        xh[1][j] = hi;
        xl[1][j] = (__bf16)(v - (float)hi);
    }
    // activations: the k-step fragments of up to 256 features
    actor_bf16x8 hin[2 * ACTOR_TILES], hout[2 * ACTOR_TILES];
    #pragma unroll
    for (int s = 0; s < 2 * ACTOR_TILES; ++s) hin[s] = hout[s] = fzero;
    // layer 1: W1 x_hi + W1 x_lo, the same two fragments
    {
        const char *w = lds + ak.w_off[0];
        const float *bias = reinterpret_cast<const float *>(lds + ak.b_off[0]);
        #pragma unroll
        for (int T = 0; T < ACTOR_TILES; ++T) {
            if (T < ak.tiles[0]) {
                const actor_bf16x8 a0 = actor_frag(w, 2 * T, lane), a1 = actor_frag(w, 2 * T + 1, lane);
                actor_f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xh[0], zero, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xh[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xl[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xl[1], acc, 0, 0, 0);
                actor_activate(acc, bias, T, h, hin[2 * T], hin[2 * T + 1]);
            }
        }
    }
    // the further hidden layers
    #pragma unroll
    for (int l = 1; l < CTR_ACTOR_MAX_HIDDEN; ++l) {
        if (l < ak.n_hidden) {
            const char *w = lds + ak.w_off[l];
            const float *bias = reinterpret_cast<const float *>(lds + ak.b_off[l]);
            const int tin = ak.tiles[l - 1];
            #pragma unroll
            for (int T = 0; T < ACTOR_TILES; ++T) {
                if (T < ak.tiles[l]) {
                    actor_f32x16 acc = zero;
                    #pragma unroll
                    for (int t = 0; t < ACTOR_TILES; ++t) {
                        if (t < tin) {
                            #pragma unroll
                            for (int s = 2 * t; s < 2 * t + 2; ++s)
                                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(actor_frag(w, T * 2 * tin + s, lane), hin[s],
                                                                              acc, 0, 0, 0);
                        }
                    }
                    actor_activate(acc, bias, T, h, hout[2 * T], hout[2 * T + 1]);
                }
            }
            #pragma unroll
            for (int s = 0; s < 2 * ACTOR_TILES; ++s) hin[s] = hout[s];
        }
    }
    // the output layer: one tile, rows 0..5 (the critic: row 0); its bias is added before the lanes move
    actor_f32x16 acc = zero;
    {
        const int lo = ak.n_hidden;               // 1..3: the offsets by constant index
        const uint32_t wo = lo == 1 ? ak.w_off[1] : (lo == 2 ? ak.w_off[2] : ak.w_off[3]);
        const uint32_t bo = lo == 1 ? ak.b_off[1] : (lo == 2 ? ak.b_off[2] : ak.b_off[3]);
        const int tin = lo == 1 ? ak.tiles[0] : (lo == 2 ? ak.tiles[1] : ak.tiles[2]);
        const char *w = lds + wo;
        #pragma unroll
        for (int t = 0; t < ACTOR_TILES; ++t) {
            if (t < tin) {
                #pragma unroll
                for (int s = 2 * t; s < 2 * t + 2; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(actor_frag(w, s, lane), hin[s], acc, 0, 0, 0);
            }
        }
        const float4 bb = *reinterpret_cast<const float4 *>(lds + bo + 16 * h);
        acc[0] += bb.x;
        acc[1] += bb.y;
        acc[2] += bb.z;
        acc[3] += bb.w;
    }
    return acc;
}

// The whole actor for the wave's 64 envs, one 32-env column tile after the other (the two tiles
// together would hold twice the activations in registers: k_rollout then spills to scratch).
// Every lane of the wave calls it: x as actor_tile<20> takes it.  Returns the lane's env's six
// pre-tanh outputs in y.
__device__ __forceinline__ void actor_logits(const ActorK &ak, const char *lds, const float x[20], float y[6])
{
    const int lane = (int)(threadIdx.x & 63), h = lane >> 5, r = lane & 31;
    #pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = 0.f;
    #pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const actor_f32x16 acc = actor_tile<20>(ak, lds, x, c);
        // rows 0..3 of env 32c + r sit on lane r, rows 4..5 on lane 32 + r; the env's own lane is
        // lane 32c + r
        #pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float v = __shfl(acc[i & 3], i < 4 ? r : 32 + r);
            y[i] = h == c ? v : y[i];
        }
    }
}

// ... and its actions in act.
__device__ __forceinline__ void actor_wave(const ActorK &ak, const char *lds, const float x[20], float act[6], float y[6])
{
    actor_logits(ak, lds, x, y);
    #pragma unroll
    for (int i = 0; i < 6; ++i) act[i] = ak.scale[i] * tanhf(y[i]);
}

// The critic's input of an env: its flat row (row[19] = 0 for one system) and the six normalised
// actions behind it, [row, a], 25 or 26 floats (x[25] = 0 for one system).
__device__ __forceinline__ void critic_row(const float row[20], const float a[6], bool multi, float x[26])
{
    #pragma unroll
    for (int k = 0; k < 19; ++k) x[k] = row[k];
    x[19] = multi ? row[19] : a[0];
    #pragma unroll
    for (int i = 0; i < 5; ++i) x[20 + i] = multi ? a[i] : a[i + 1];
    x[25] = multi ? a[5] : 0.f;
}

// The whole critic for the wave's 64 rows, as actor_logits: x as actor_tile<26> takes it.  Returns
// the lane's row's Q (row 0 of the output tile: register 0 of lane r).
__device__ __forceinline__ float critic_wave(const ActorK &ck, const char *lds, const float x[26])
{
    const int lane = (int)(threadIdx.x & 63), h = lane >> 5, r = lane & 31;
    float q = 0.f;
    #pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const actor_f32x16 acc = actor_tile<26>(ck, lds, x, c);
        const float v = __shfl(acc[0], r);
        q = h == c ? v : q;
    }
    return q;
}
