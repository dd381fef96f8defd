// ctr_ddpg.inc -- DDPG's two updates on the learner's float32 parameters (ctr_ddpg_critic_step,
// ctr_ddpg_actor_step), with their extern "C" entry points.  Included at the end of
// ctr_kernels.hip, after ctr_polyak.inc.
//
// Restates the update of stable-baselines DDPG (ddpg.py _train_step) as the example trains it: the
// critic's regression on the target, the policy's ascent on Q(s, pi(s)), each followed by one Adam
// step.  Everything is float32 (but the two f64 row sums at DdpgNetK); the bf16 blobs are not read.
//
// Two launches per step.  k_ddpg_grad: a workgroup takes tiles of DDPG_T = 16 rows (tile, tile +
// grid, ...), keeps the tile's activations in LDS between forward and backward, and adds the
// tile's weight gradients to its own slot of the workspace, so slot s holds the sum over its tiles
// in tile order.  k_ddpg_apply: one thread per parameter sums the slots in slot order, stores the
// gradient and makes the Adam step.  No atomics, nobody waits for anybody, and the order of every
// sum is a function of the shapes and B alone.
//
// ctr_td3_critic_step makes the critic's step for TD3's two critics in the same two launches: the
// grids get a second dimension, plane blockIdx.y works on critic y with its own arguments and its
// own region of the workspace, and the kernels' bodies are device functions both pairs call.
//
// The products run on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: a chain of fmaf at exact
// f32).  Lane (c = lane & 15, g = lane >> 4) gives A[i = c][k = g] and B[k = g][j = c] and holds
// D[i = 4 g + reg][j = c].  A k-block of 16 is four MFMAs; in MFMA t lane group g supplies
// k = 4 g + t, so that each lane reads its four k as one 16-B load.
//     forward   Y[r][o]  = sum_k X[r][k] W[o][k]       A = X (LDS),      B = W (global)
//     backward  dX[r][k] = sum_o dZ[r][o] W[o][k]      A = dZ (LDS),     B = W (global)
//               dW[o][k] = sum_r dZ[r][o] H[r][k]      A = dZ^T (LDS),   B = H (LDS), C = the slot
// dZ[l] overwrites H[l] in place (the relu mask is H[l] > 0, read by the lane that writes), so a
// network needs one LDS image of its activations and nothing else.
namespace {

typedef float ddpg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int DDPG_T = 16;                       // rows of a tile
constexpr int DDPG_SLOTS = 64;                   // partial sums per parameter, at most
constexpr int DDPG_PAD = 4;                      // floats behind every LDS row (the rows stay 16-B aligned)
constexpr int DDPG_X0 = 32;                      // the input row, zero-padded
constexpr int DDPG_OUTC = 16;                    // the output layer's columns, zero-padded
constexpr int DDPG_TENSORS = 2 * ACTOR_LAYERS;
constexpr size_t DDPG_HDR = 16 + DDPG_SLOTS * sizeof(double);  // the advanced pow[2]; the loss partials (f64)
constexpr int64_t DDPG_MAX_B = 65536;

// A network's float32 parameters with its shape; the flat order of the parameters, and of a workspace
// slot's floats, is W[0], b[0], W[1], b[1], ...  The two sums over rows whose terms cancel -- the loss
// and the bias gradients -- are accumulated in f64 and rounded to f32 once (a sequential f32 sum of B
// terms loses about 1e-7 of the result, several times what the forward pass does): a slot keeps its
// bias sums as doubles behind its floats, in the order b[0], b[1], ..., and the b[l] floats unused.
struct DdpgNetK {
    int32_t in_dim, n_hidden, out_rows, params, biases;
    int32_t boff[ACTOR_LAYERS];        // b[l]'s first double among a slot's bias sums
    int32_t width[CTR_ACTOR_MAX_HIDDEN];
    int32_t off[ACTOR_LAYERS];         // W[l]'s first float in a slot; b[l] follows it
    const float *W[ACTOR_LAYERS], *b[ACTOR_LAYERS];
};

__host__ __device__ inline int ddpg_rows(const DdpgNetK &n, int l)
{
    return l < CTR_ACTOR_MAX_HIDDEN && l < n.n_hidden ? n.width[l < CTR_ACTOR_MAX_HIDDEN ? l : 0] : n.out_rows;
}

__host__ __device__ inline int ddpg_cols(const DdpgNetK &n, int l)
{
    return l == 0 ? n.in_dim : n.width[l - 1 < CTR_ACTOR_MAX_HIDDEN && l > 0 ? l - 1 : 0];
}

// floats of a slot's weight sums (a multiple of 4: the doubles behind them are 16-B aligned), and of the whole slot
__host__ __device__ inline int64_t ddpg_slot_w(int params) { return ((int64_t)params + 3) & ~(int64_t)3; }
__host__ __device__ inline int64_t ddpg_slot_floats(int params, int biases)
{
    return ddpg_slot_w(params) + ((2 * (int64_t)biases + 3) & ~(int64_t)3);
}

inline int64_t ddpg_slots_for(int64_t B) { return std::min<int64_t>((B + DDPG_T - 1) / DDPG_T, DDPG_SLOTS); }

inline int64_t ddpg_ws_bytes(int params, int biases, int64_t B)
{
    return (int64_t)DDPG_HDR + ddpg_slots_for(B) * ddpg_slot_floats(params, biases) * (int64_t)sizeof(float);
}

// The LDS image of a network's tile: the input rows, every hidden layer, the output layer.
struct DdpgLds {
    float *x0, *h[CTR_ACTOR_MAX_HIDDEN], *out;
};

__host__ __device__ inline int ddpg_lds_floats(const DdpgNetK &n)
{
    int f = DDPG_T * (DDPG_X0 + DDPG_PAD) + DDPG_T * (DDPG_OUTC + DDPG_PAD);
    for (int l = 0; l < CTR_ACTOR_MAX_HIDDEN; ++l)
        if (l < n.n_hidden) f += DDPG_T * (n.width[l] + DDPG_PAD);
    return f;
}

__device__ __forceinline__ float *ddpg_lds_net(const DdpgNetK &n, float *base, DdpgLds &L)
{
    L.x0 = base;
    base += DDPG_T * (DDPG_X0 + DDPG_PAD);
    #pragma unroll
    for (int l = 0; l < CTR_ACTOR_MAX_HIDDEN; ++l) {
        L.h[l] = base;
        if (l < n.n_hidden) base += DDPG_T * (n.width[l] + DDPG_PAD);
    }
    L.out = base;
    return base + DDPG_T * (DDPG_OUTC + DDPG_PAD);
}

// Y = X W^T + b (relu: the hidden layers).  first: layer 0, whose K = in_dim real columns are read
// one by one (a row of 19..26 floats is not 16-B aligned) under X's 32 padded ones.
__device__ __forceinline__ void ddpg_layer_fwd(const float *W, const float *b, int rows, int K, bool first,
                                               const float *X, int sx, float *Y, int sy, bool relu)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), c = lane & 15, g = lane >> 4;
    const int Kp = first ? DDPG_X0 : K;
    const int ntile = (rows + 15) >> 4;
    for (int tile = wave; tile < ntile; tile += BLOCK / 64) {
        const int o = 16 * tile + c;
        // four chains, one per t, added pairwise at the end: a quarter of the roundings on any path of
        // one k-ordered chain (a single chain over K = 32 .. 256 loses about twice what a blocked CPU
        // GEMM does, and the mean of Q shows it), and independent MFMAs back to back
        ddpg_f32x4 acc4[4];
        #pragma unroll
        for (int t = 0; t < 4; ++t) acc4[t] = ddpg_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < Kp; s += 16) {
            const int k = s + 4 * g;
            const ddpg_f32x4 a = *reinterpret_cast<const ddpg_f32x4 *>(X + c * sx + k);
            ddpg_f32x4 w = {0.f, 0.f, 0.f, 0.f};
            if (o < rows) {
                const float *wr = W + (size_t)o * K;
                if (first) {
                    #pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (k + t < K) w[t] = wr[k + t];
                } else {
                    const actor_f32x4u v = *reinterpret_cast<const actor_f32x4u *>(wr + k);
                    w = ddpg_f32x4{v[0], v[1], v[2], v[3]};
                }
            }
            #pragma unroll
            for (int t = 0; t < 4; ++t) acc4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], w[t], acc4[t], 0, 0, 0);
        }
        const ddpg_f32x4 acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
        const float bias = o < rows ? b[o] : 0.f;
        #pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float z = acc[reg] + bias;
            if (relu) z = z > 0.f ? z : 0.f;
            Y[(4 * g + reg) * sy + o] = z;
        }
    }
}

// dX = dZ W over the column tiles tile0 .. ntile - 1 of X, stored over H: masked by H > 0 (a hidden
// layer: dZ of the layer below) or plain (the input row).  Op: dZ's columns, padded to whole 16.
__device__ __forceinline__ void ddpg_layer_dx(const float *W, int rows, int K, const float *dZ, int sz, int Op,
                                              float *H, int sh, int tile0, int ntile, bool mask)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), c = lane & 15, g = lane >> 4;
    for (int tile = tile0 + wave; tile < ntile; tile += BLOCK / 64) {
        const int kcol = 16 * tile + c;
        ddpg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < Op; s += 16) {
            const int o = s + 4 * g;
            const ddpg_f32x4 a = *reinterpret_cast<const ddpg_f32x4 *>(dZ + c * sz + o);
            ddpg_f32x4 w = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int t = 0; t < 4; ++t)
                if (o + t < rows && kcol < K) w[t] = W[(size_t)(o + t) * K + kcol];
            #pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], w[t], acc, 0, 0, 0);
        }
        #pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float *p = H + (4 * g + reg) * sh + kcol;
            *p = !mask || *p > 0.f ? acc[reg] : 0.f;
        }
    }
}

// The tile's dW = dZ^T H and db = the column sums of dZ, added to the slot (first: the slot's first
// tile starts it).  Each element of the slot belongs to one thread for the whole launch.
__device__ __forceinline__ void ddpg_layer_dw(const float *dZ, int sz, int rows, const float *H, int sh, int K, int Kp,
                                              float *gW, double *gb, bool first)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), c = lane & 15, g = lane >> 4;
    const int kt = Kp >> 4, ntile = ((rows + 15) >> 4) * kt;
    for (int tile = wave; tile < ntile; tile += BLOCK / 64) {
        const int to = tile / kt, tk = tile - to * kt;
        const int k = 16 * tk + c;
        ddpg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (!first && k < K) {
            #pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = 16 * to + 4 * g + reg;
                if (o < rows) acc[reg] = gW[(size_t)o * K + k];
            }
        }
        #pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = 4 * t + g;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dZ[r * sz + 16 * to + c], H[r * sh + k], acc, 0, 0, 0);
        }
        if (k < K) {
            #pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = 16 * to + 4 * g + reg;
                if (o < rows) gW[(size_t)o * K + k] = acc[reg];
            }
        }
    }
    for (int o = (int)threadIdx.x; o < rows; o += BLOCK) {
        double s = first ? 0.0 : gb[o];
        #pragma unroll
        for (int r = 0; r < DDPG_T; ++r) s += (double)dZ[r * sz + o];
        gb[o] = s;
    }
}

// Every layer of a network on the tile in L.x0; a barrier follows each layer.
__device__ __forceinline__ void ddpg_forward(const DdpgNetK &n, const DdpgLds &L)
{
    #pragma unroll
    for (int l = 0; l < ACTOR_LAYERS; ++l) {
        if (l <= n.n_hidden) {
            const bool last = l == n.n_hidden;
            const int rows = ddpg_rows(n, l), K = ddpg_cols(n, l);
            const float *X = l == 0 ? L.x0 : L.h[l > 0 ? l - 1 : 0];
            float *Y = last ? L.out : L.h[l < CTR_ACTOR_MAX_HIDDEN ? l : 0];
            ddpg_layer_fwd(n.W[l], n.b[l], rows, K, l == 0, X, (l == 0 ? DDPG_X0 : K) + DDPG_PAD, Y,
                           (last ? DDPG_OUTC : rows) + DDPG_PAD, !last);
            __syncthreads();
        }
    }
}

// From dZ of the output layer in L.out (its columns past out_rows zero) down to layer 0.  grads:
// every layer's dW and db go to the slot; otherwise (the critic under the actor's loss) only dX is
// made, and that of layer 0 is stored plain over the input row's column tiles from x_tile0 on.
// Ends with a barrier.
__device__ __forceinline__ void ddpg_backward(const DdpgNetK &n, const DdpgLds &L, bool grads, float *slot, bool first,
                                              int x_tile0)
{
    #pragma unroll
    for (int l = ACTOR_LAYERS - 1; l >= 0; --l) {
        if (l <= n.n_hidden) {
            const bool last = l == n.n_hidden;
            const int rows = ddpg_rows(n, l), K = ddpg_cols(n, l);
            const float *dZ = last ? L.out : L.h[l < CTR_ACTOR_MAX_HIDDEN ? l : 0];
            const int sz = (last ? DDPG_OUTC : rows) + DDPG_PAD, Op = last ? DDPG_OUTC : rows;
            float *H = l == 0 ? L.x0 : L.h[l > 0 ? l - 1 : 0];
            const int sh = (l == 0 ? DDPG_X0 : K) + DDPG_PAD;
            if (grads) {
                float *gW = slot + n.off[l];
                double *gb = reinterpret_cast<double *>(slot + ddpg_slot_w(n.params)) + n.boff[l];
                ddpg_layer_dw(dZ, sz, rows, H, sh, K, l == 0 ? DDPG_X0 : K, gW, gb, first);
                __syncthreads();
            }
            if (l > 0) ddpg_layer_dx(n.W[l], rows, K, dZ, sz, Op, H, sh, 0, K >> 4, true);
            else if (!grads) ddpg_layer_dx(n.W[0], rows, K, dZ, sz, Op, H, sh, x_tile0, DDPG_X0 >> 4, false);
            __syncthreads();
        }
    }
}

struct DdpgGradK {
    DdpgNetK net;                      // the network that learns
    DdpgNetK crit;                     // the actor's step: the critic, read only
    const float *rows, *actions, *scale, *target;
    int32_t B;
    float dq;                          // dL/dq of a row: 2/B times (q - target), or -1/B
    float beta1, beta2;
    const float *pow;
    char *ws;
};

// The gradient launch's work of one workgroup (slot blockIdx.x of k.ws); s_loss: DDPG_T floats of LDS.
template <bool ACTOR>
__device__ __forceinline__ void ddpg_grad_block(const DdpgGradK &k, float *s_loss)
{
    float *lds = reinterpret_cast<float *>(actor_lds_base(0));
    DdpgLds La = {}, Lc = {};
    if (ACTOR) lds = ddpg_lds_net(k.net, lds, La);
    ddpg_lds_net(ACTOR ? k.crit : k.net, lds, Lc);
    const DdpgNetK &cn = ACTOR ? k.crit : k.net;
    const int row_dim = cn.in_dim - 6;             // the actor's in_dim
    float *hdr = reinterpret_cast<float *>(k.ws);
    float *slot = reinterpret_cast<float *>(k.ws + DDPG_HDR) +
                  (size_t)blockIdx.x * ddpg_slot_floats(k.net.params, k.net.biases);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the powers this step's Adam divides by: k_ddpg_apply reads these and stores them to pow
        hdr[0] = k.pow[0] * k.beta1;
        hdr[1] = k.pow[1] * k.beta2;
    }
    const int ntiles = (k.B + DDPG_T - 1) / DDPG_T;
    double lsum = 0.0;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x, first = false) {
        const int r0 = tile * DDPG_T;
        // the tile's input rows, zero past B and past in_dim
        for (int i = (int)threadIdx.x; i < DDPG_T * DDPG_X0; i += BLOCK) {
            const int r = i / DDPG_X0, c = i - r * DDPG_X0;
            const bool valid = r0 + r < k.B;
            const float x = valid && c < row_dim ? k.rows[(size_t)(r0 + r) * row_dim + c] : 0.f;
            float xc = x;
            if (!ACTOR && valid && c >= row_dim && c < cn.in_dim) {
                xc = k.actions[(size_t)(r0 + r) * 6 + (c - row_dim)];
                if (k.scale) xc = xc / k.scale[c - row_dim];
            }
            if (ACTOR) La.x0[r * (DDPG_X0 + DDPG_PAD) + c] = x;
            Lc.x0[r * (DDPG_X0 + DDPG_PAD) + c] = xc;
        }
        __syncthreads();
        if (ACTOR) {
            ddpg_forward(k.net, La);
            if (threadIdx.x < DDPG_T * 6) {
                const int r = (int)threadIdx.x / 6, j = (int)threadIdx.x - 6 * r;
                // tanh rounded to f32 once: the device's tanhf is off by up to 2 ulp, not evenly to both sides,
                // and mean Q over a batch shows that
                const float a = (float)tanh((double)La.out[r * (DDPG_OUTC + DDPG_PAD) + j]);
                La.out[r * (DDPG_OUTC + DDPG_PAD) + j] = a;
                Lc.x0[r * (DDPG_X0 + DDPG_PAD) + row_dim + j] = a;
            }
            __syncthreads();
        }
        ddpg_forward(cn, Lc);
        if (threadIdx.x < DDPG_T) {
            const int r = (int)threadIdx.x;
            const bool valid = r0 + r < k.B;
            float *q = Lc.out + r * (DDPG_OUTC + DDPG_PAD);
            if (ACTOR) {
                s_loss[r] = valid ? *q : 0.f;
                *q = valid ? k.dq : 0.f;
            } else {
                const float d = valid ? *q - k.target[r0 + r] : 0.f;
                s_loss[r] = d * d;
                *q = d * k.dq;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            #pragma unroll
            for (int r = 0; r < DDPG_T; ++r) lsum += (double)s_loss[r];
        if (ACTOR) {
            ddpg_backward(k.crit, Lc, false, nullptr, first, row_dim >> 4);
            if (threadIdx.x < DDPG_T * 6) {
                const int r = (int)threadIdx.x / 6, j = (int)threadIdx.x - 6 * r;
                float *y = La.out + r * (DDPG_OUTC + DDPG_PAD) + j;
                const float a = *y;
                *y = Lc.x0[r * (DDPG_X0 + DDPG_PAD) + row_dim + j] * (1.f - a * a);
            }
            __syncthreads();
        }
        ddpg_backward(k.net, ACTOR ? La : Lc, true, slot, first, 0);
    }
    if (threadIdx.x == 0) reinterpret_cast<double *>(k.ws + 16)[blockIdx.x] = lsum;
}

template <bool ACTOR>
__global__ __launch_bounds__(BLOCK) void k_ddpg_grad(DdpgGradK k)
{
    __shared__ float s_loss[DDPG_T];
    ddpg_grad_block<ACTOR>(k, s_loss);
}

// TD3's two critics in one launch: plane blockIdx.y of the grid is k_ddpg_grad<false> on critic y,
// with its own arguments and its own region of the workspace.  The branch is wave-uniform, and each
// side reads its struct by constant offsets.
__global__ __launch_bounds__(BLOCK) void k_td3_grad(DdpgGradK k0, DdpgGradK k1)
{
    __shared__ float s_loss[DDPG_T];
    if (blockIdx.y == 0) ddpg_grad_block<false>(k0, s_loss);
    else ddpg_grad_block<false>(k1, s_loss);
}

struct DdpgApplyK {
    int32_t params, biases, slots;
    int32_t end[DDPG_TENSORS];         // the flat order's tensor ends (past the network: params)
    int32_t boff[ACTOR_LAYERS];        // as DdpgNetK's
    float *p[DDPG_TENSORS], *g[DDPG_TENSORS], *m[DDPG_TENSORS], *v[DDPG_TENSORS];
    float lr, beta1, beta2, eps;
    double loss_scale;                 // 1/B, or -1/B
    float *pow, *loss;
    const char *ws;
};

// One Adam step of an element, every operation rounded to f32 (no fused multiply-add): numpy's
// float32 arithmetic, bit for bit.  pw1, pw2: beta1^t, beta2^t of this step.
__device__ __forceinline__ float ddpg_adam(float p, float g, float &m, float &v, float lr, float b1, float b2, float eps,
                                           float pw1, float pw2)
{
#pragma clang fp contract(off)
    const float mo = b1 * m, mg = (1.0f - b1) * g;
    m = mo + mg;
    const float vo = b2 * v, vg = ((1.0f - b2) * g) * g;
    v = vo + vg;
    const float mh = m / (1.0f - pw1), vh = v / (1.0f - pw2);
    const float den = sqrtf(vh) + eps;
    const float step = lr * (mh / den);
    return p - step;
}

// Element 0's duties behind a gradient launch, in the apply kernels and in the update calls' tails
// (ctr_sac_update.inc, ctr_ddpg_update.inc): the advanced powers to pow, and the slots' loss partials,
// summed in slot order and scaled, to loss and to a history entry (either may be NULL; hist by reference:
// a tail's is a kernel argument, read where it is used).
__device__ __forceinline__ void ddpg_apply_head(const DdpgApplyK &k, float *const &hist, float pw1, float pw2)
{
    k.pow[0] = pw1;
    k.pow[1] = pw2;
    if (k.loss || hist) {
        const double *lpart = reinterpret_cast<const double *>(k.ws + 16);
        double s = lpart[0];
        for (int t = 1; t < k.slots; ++t) s += lpart[t];
        const float loss = (float)(s * k.loss_scale);
        if (k.loss) *k.loss = loss;
        if (hist) *hist = loss;
    }
}

// The apply launch's work of one thread: element blockIdx.x * BLOCK + threadIdx.x of k's network.
__device__ __forceinline__ void ddpg_apply_element(const DdpgApplyK &k)
{
    const float *hdr = reinterpret_cast<const float *>(k.ws);
    const float *part = reinterpret_cast<const float *>(k.ws + DDPG_HDR);
    const int64_t stride = ddpg_slot_floats(k.params, k.biases);
    const int e = (int)(blockIdx.x * BLOCK + threadIdx.x);
    const float pw1 = hdr[0], pw2 = hdr[1];
    if (e == 0) ddpg_apply_head(k, nullptr, pw1, pw2);
    if (e >= k.params) return;
    // the element's tensor; the arrays by constant index (they are kernel arguments)
    int firstf = 0, tensor = 0;
    float *p = k.p[0], *gp = k.g[0], *mp = k.m[0], *vp = k.v[0];
    #pragma unroll
    for (int t = 0; t + 1 < DDPG_TENSORS; ++t)
        if (e >= k.end[t]) {
            firstf = k.end[t];
            tensor = t + 1;
            p = k.p[t + 1];
            gp = k.g[t + 1];
            mp = k.m[t + 1];
            vp = k.v[t + 1];
        }
    const int i = e - firstf;
    float g;
    if (tensor & 1) {
        // a bias: the slots' f64 sums, rounded once
        int bo = k.boff[0];
        #pragma unroll
        for (int l = 1; l < ACTOR_LAYERS; ++l)
            if (tensor == 2 * l + 1) bo = k.boff[l];
        const double *bp = reinterpret_cast<const double *>(part + ddpg_slot_w(k.params)) + bo + i;
        double s = bp[0];
        for (int j = 1; j < k.slots; ++j) s += bp[(size_t)j * (stride / 2)];
        g = (float)s;
    } else {
        g = part[e];
        for (int j = 1; j < k.slots; ++j) g += part[(size_t)j * stride + e];
    }
    float m = mp[i], v = vp[i];
    gp[i] = g;
    p[i] = ddpg_adam(p[i], g, m, v, k.lr, k.beta1, k.beta2, k.eps, pw1, pw2);
    mp[i] = m;
    vp[i] = v;
}

__global__ __launch_bounds__(BLOCK) void k_ddpg_apply(DdpgApplyK k) { ddpg_apply_element(k); }

// k_ddpg_apply on TD3's two critics: plane blockIdx.y applies critic y's slots (the grid's x is the
// larger network's; the threads past a network's parameters leave as in k_ddpg_apply).
__global__ __launch_bounds__(BLOCK) void k_td3_apply(DdpgApplyK k0, DdpgApplyK k1)
{
    if (blockIdx.y == 0) ddpg_apply_element(k0);
    else ddpg_apply_element(k1);
}

int ddpg_fail(const char *fn, const char *why)
{
    snprintf(g_err, sizeof g_err, "%s: %s", fn, why);
    return CTR_EINVAL;
}

// The shape part of a DdpgNetK from a checked layout.
void ddpg_shape(const ActorK &ak, DdpgNetK *nk)
{
    memset(nk, 0, sizeof *nk);
    nk->in_dim = ak.in_dim;
    nk->n_hidden = ak.n_hidden;
    nk->out_rows = ak.out_rows;
    for (int l = 0; l < ak.n_hidden; ++l) nk->width[l] = 32 * ak.tiles[l];
    int off = 0, boff = 0;
    for (int l = 0; l <= ak.n_hidden; ++l) {
        nk->off[l] = off;
        nk->boff[l] = boff;
        off += ddpg_rows(*nk, l) * (ddpg_cols(*nk, l) + 1);
        boff += ddpg_rows(*nk, l);
    }
    nk->params = off;
    nk->biases = boff;
}

int ddpg_shape_check(const char *fn, const ctr_actor_t *a, const ctr_critic_t *c, bool need_actor, DdpgNetK *an, DdpgNetK *cn)
{
    ActorK ak;
    if (need_actor || a) {
        if (!a) return ddpg_fail(fn, "actor is NULL");
        if (actor_layout(a, &ak)) {
            char why[sizeof g_err];
            snprintf(why, sizeof why, "%s", g_err);
            snprintf(g_err, sizeof g_err, "%s: %.400s", fn, why);
            return CTR_EINVAL;
        }
        ddpg_shape(ak, an);
    }
    if (!c) return ddpg_fail(fn, "critic is NULL");
    if (critic_layout(c, &ak)) {
        char why[sizeof g_err];
        snprintf(why, sizeof why, "%s", g_err);
        snprintf(g_err, sizeof g_err, "%s: %.400s", fn, why);
        return CTR_EINVAL;
    }
    ddpg_shape(ak, cn);
    if ((need_actor || a) && an->in_dim + 6 != cn->in_dim) return ddpg_fail(fn, "actor->in_dim + 6 must be critic->in_dim");
    return 0;
}

// The learning network's tensors, the Adam constants, B and the workspace: fills nk's pointers and ap.
int ddpg_learn_check(const char *fn, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam, int64_t B, void *workspace,
                     int64_t workspace_bytes, DdpgNetK *nk, DdpgApplyK *ap)
{
    if (!net) return ddpg_fail(fn, "net is NULL");
    if (!adam) return ddpg_fail(fn, "adam is NULL");
    if (!net->W || !net->b || !net->gW || !net->gb || !net->mW || !net->mb || !net->vW || !net->vb || !net->pow)
        return ddpg_fail(fn, "NULL pointer array or pow in net");
    memset(ap, 0, sizeof *ap);
    for (int l = 0; l <= nk->n_hidden; ++l) {
        float *const t[8] = {net->W[l], net->b[l], net->gW[l], net->gb[l], net->mW[l], net->mb[l], net->vW[l], net->vb[l]};
        for (int i = 0; i < 8; ++i)
            if (!t[i]) return ddpg_fail(fn, "NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]");
        nk->W[l] = net->W[l];
        nk->b[l] = net->b[l];
        for (int h = 0; h < 2; ++h) {
            ap->p[2 * l + h] = t[h];
            ap->g[2 * l + h] = t[2 + h];
            ap->m[2 * l + h] = t[4 + h];
            ap->v[2 * l + h] = t[6 + h];
        }
        ap->end[2 * l] = nk->off[l] + ddpg_rows(*nk, l) * ddpg_cols(*nk, l);
        ap->end[2 * l + 1] = ap->end[2 * l] + ddpg_rows(*nk, l);
    }
    const int nt = 2 * (nk->n_hidden + 1);
    for (int t = nt; t < DDPG_TENSORS; ++t) ap->end[t] = nk->params;
    for (int t = 0; t < nt; ++t)
        for (int u = 0; u < nt; ++u)
            if (ap->g[t] == ap->p[u] || ap->m[t] == ap->p[u] || ap->v[t] == ap->p[u] || net->pow == ap->p[u])
                return ddpg_fail(fn, "a gradient or state tensor is a parameter tensor");
    if (!isfinite(adam->lr) || !isfinite(adam->beta1) || !isfinite(adam->beta2) || !isfinite(adam->eps))
        return ddpg_fail(fn, "lr, beta1, beta2 and eps must be finite");
    if (!(adam->beta1 >= 0.f && adam->beta1 < 1.f && adam->beta2 >= 0.f && adam->beta2 < 1.f))
        return ddpg_fail(fn, "beta1 and beta2 must be in [0, 1)");
    if (!(adam->eps > 0.f)) return ddpg_fail(fn, "eps must be positive");
    if (B < 0 || B > DDPG_MAX_B) return ddpg_fail(fn, "B must be in 0..65536");
    if (!workspace) return ddpg_fail(fn, "workspace is NULL");
    if (((uintptr_t)workspace & 15u) != 0) return ddpg_fail(fn, "workspace must be 16-B aligned");
    if (workspace_bytes < ddpg_ws_bytes(nk->params, nk->biases, B))
        return ddpg_fail(fn, "workspace too small (ctr_ddpg_workspace_bytes)");
    ap->params = nk->params;
    ap->biases = nk->biases;
    for (int l = 0; l < ACTOR_LAYERS; ++l) ap->boff[l] = nk->boff[l];
    ap->slots = (int32_t)ddpg_slots_for(B);
    ap->lr = adam->lr;
    ap->beta1 = adam->beta1;
    ap->beta2 = adam->beta2;
    ap->eps = adam->eps;
    ap->pow = net->pow;
    ap->ws = static_cast<const char *>(workspace);
    return 0;
}

// The critics of a step (nc: 1, or 2 for the twins), each entry in turn: its shape, then the two of one
// in_dim; critic 0's workspace region as ctr_ddpg_critic_step lays it out, critic 1's behind it (a region
// is a multiple of 16 B), and ddpg_learn_check on each.  null_entry: the caller's words for a NULL
// critic[y] or net[y] (reached from ctr_ddpg_update only, which looks at entry and shape critic by critic; the
// twin callers have refused a NULL entry of either critic before they call); twin_ws: the workspace
// function its message names when the second region does not fit.
int ddpg_critics_check(const char *fn, int nc, const ctr_critic_t *const *critic, const ctr_ddpg_net_t *const *net,
                       const ctr_ddpg_adam_t *adam, int64_t B, void *workspace, int64_t workspace_bytes,
                       const char *null_entry, const char *twin_ws, DdpgGradK *gk, DdpgApplyK *ap)
{
    static_assert(DDPG_HDR % 16 == 0, "a region is a multiple of 16 B");
    for (int y = 0; y < nc; ++y) {
        if (!critic[y] || !net[y]) return ddpg_fail(fn, null_entry);
        if (int r = ddpg_shape_check(fn, nullptr, critic[y], false, nullptr, &gk[y].net)) return r;
    }
    if (nc == 2 && gk[0].net.in_dim != gk[1].net.in_dim) return ddpg_fail(fn, "the two critics must have the same in_dim");
    const int64_t Bc = B < 0 ? 0 : std::min(B, DDPG_MAX_B);
    const int64_t off = ddpg_ws_bytes(gk[0].net.params, gk[0].net.biases, Bc);
    if (int r = ddpg_learn_check(fn, net[0], adam, B, workspace, workspace_bytes, &gk[0].net, &ap[0])) return r;
    if (nc == 1) return 0;
    if (workspace_bytes < off + ddpg_ws_bytes(gk[1].net.params, gk[1].net.biases, Bc)) return ddpg_fail(fn, twin_ws);
    return ddpg_learn_check(fn, net[1], adam, B, static_cast<char *>(workspace) + off, workspace_bytes - off, &gk[1].net, &ap[1]);
}

// What a gradient launch (DdpgGradK, SacGradK) takes from its network's checked DdpgApplyK.
template <class GradK>
void ddpg_grad_state(GradK &gk, const DdpgApplyK &ap)
{
    gk.beta1 = ap.beta1;
    gk.beta2 = ap.beta2;
    gk.pow = ap.pow;
    gk.ws = const_cast<char *>(ap.ws);
}

// A checked critic's launch arguments for a batch of B > 0 rows -> the dynamic LDS bytes of its gradient launch.
size_t ddpg_critic_fill(DdpgGradK &gk, DdpgApplyK &ap, const float *rows, const float *actions, const float *scale,
                        const float *target, int64_t B, float *loss)
{
    gk.rows = rows;
    gk.actions = actions;
    gk.scale = scale;
    gk.target = target;
    gk.B = (int32_t)B;
    gk.dq = (float)(2.0 / (double)B);
    ddpg_grad_state(gk, ap);
    ap.loss_scale = 1.0 / (double)B;
    ap.loss = loss;
    return ddpg_lds_floats(gk.net) * sizeof(float) + ACTOR_LDS_SLACK;
}

// The two launches of a single step; shm: the gradient launch's dynamic LDS bytes.
template <bool ACTOR>
int ddpg_launch(const char *fn, const DdpgGradK &gk, const DdpgApplyK &ap, size_t shm, void *stream)
{
    constexpr size_t MAX_SHM = 2 * (size_t)DDPG_T * (DDPG_X0 + DDPG_OUTC + 2 * DDPG_PAD + CTR_ACTOR_MAX_HIDDEN *
                                                     (CTR_ACTOR_MAX_WIDTH + DDPG_PAD)) * sizeof(float) + ACTOR_LDS_SLACK;
    static_assert(MAX_SHM + DDPG_T * sizeof(float) <= LDS_PER_WORKGROUP, "every actor with every critic fits in LDS");
    if (int r = allow_dynamic_lds(k_ddpg_grad<ACTOR>, shm)) return r;
    hipLaunchKernelGGL(k_ddpg_grad<ACTOR>, dim3((unsigned)ap.slots), dim3(BLOCK), shm, (hipStream_t)stream, gk);
    hipLaunchKernelGGL(k_ddpg_apply, dim3(grid_for(ap.params)), dim3(BLOCK), 0, (hipStream_t)stream, ap);
    char what[64];
    snprintf(what, sizeof what, "%s launch", fn);
    return hip_check(what);
}

}  // namespace

extern "C" {

int64_t ctr_ddpg_workspace_bytes(const ctr_actor_t *actor, const ctr_critic_t *critic, int64_t max_B)
{
    DdpgNetK an, cn;
    if (ddpg_shape_check("ctr_ddpg_workspace_bytes", actor, critic, true, &an, &cn)) return -1;
    if (max_B < 1 || max_B > DDPG_MAX_B) {
        ddpg_fail("ctr_ddpg_workspace_bytes", "max_B must be in 1..65536");
        return -1;
    }
    return std::max(ddpg_ws_bytes(an.params, an.biases, max_B), ddpg_ws_bytes(cn.params, cn.biases, max_B));
}

int ctr_ddpg_critic_step(const ctr_critic_t *critic, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam,
                         const float *rows, const float *actions, const float *scale, const float *target, int64_t B,
                         float *loss, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "ctr_ddpg_critic_step";
    DdpgGradK gk = {};
    DdpgApplyK ap;
    if (int r = ddpg_shape_check(fn, nullptr, critic, false, nullptr, &gk.net)) return r;
    if (int r = ddpg_learn_check(fn, net, adam, B, workspace, workspace_bytes, &gk.net, &ap)) return r;
    if (B > 0 && (!rows || !actions || !target)) return ddpg_fail(fn, "rows, actions or target is NULL");
    if (B == 0) return 0;
    const size_t shm = ddpg_critic_fill(gk, ap, rows, actions, scale, target, B, loss);
    return ddpg_launch<false>(fn, gk, ap, shm, stream);
}

int ctr_ddpg_actor_step(const ctr_actor_t *actor, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam,
                        const ctr_critic_t *critic, const float *const *critic_W, const float *const *critic_b,
                        const float *rows, int64_t B, float *loss, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "ctr_ddpg_actor_step";
    DdpgGradK gk = {};
    DdpgApplyK ap;
    if (int r = ddpg_shape_check(fn, actor, critic, true, &gk.net, &gk.crit)) return r;
    if (int r = ddpg_learn_check(fn, net, adam, B, workspace, workspace_bytes, &gk.net, &ap)) return r;
    if (!critic_W || !critic_b) return ddpg_fail(fn, "critic_W or critic_b is NULL");
    for (int l = 0; l <= gk.crit.n_hidden; ++l) {
        if (!critic_W[l] || !critic_b[l]) return ddpg_fail(fn, "NULL layer among critic_W, critic_b [0..n_hidden]");
        gk.crit.W[l] = critic_W[l];
        gk.crit.b[l] = critic_b[l];
    }
    if (B > 0 && !rows) return ddpg_fail(fn, "rows is NULL");
    if (B == 0) return 0;
    gk.rows = rows;
    gk.B = (int32_t)B;
    gk.dq = (float)(-1.0 / (double)B);
    ddpg_grad_state(gk, ap);
    ap.loss_scale = -1.0 / (double)B;
    ap.loss = loss;
    const size_t shm = (ddpg_lds_floats(gk.net) + ddpg_lds_floats(gk.crit)) * sizeof(float) + ACTOR_LDS_SLACK;
    return ddpg_launch<true>(fn, gk, ap, shm, stream);
}

int64_t ctr_td3_workspace_bytes(const ctr_actor_t *actor, const ctr_critic_t *critic1, const ctr_critic_t *critic2,
                                int64_t max_B)
{
    const char *fn = "ctr_td3_workspace_bytes";
    DdpgNetK an, c1, c2;
    if (ddpg_shape_check(fn, actor, critic1, true, &an, &c1)) return -1;
    if (ddpg_shape_check(fn, actor, critic2, true, &an, &c2)) return -1;
    if (max_B < 1 || max_B > DDPG_MAX_B) {
        ddpg_fail(fn, "max_B must be in 1..65536");
        return -1;
    }
    // the two critics' regions, one behind the other (each a multiple of 16 B); or the actor's step
    const int64_t twin = ddpg_ws_bytes(c1.params, c1.biases, max_B) + ddpg_ws_bytes(c2.params, c2.biases, max_B);
    return std::max(twin, ddpg_ws_bytes(an.params, an.biases, max_B));
}

int ctr_td3_critic_step(const ctr_critic_t *const critic[2], const ctr_ddpg_net_t *const net[2],
                        const ctr_ddpg_adam_t *adam, const float *rows, const float *actions, const float *scale,
                        const float *target, int64_t B, float *loss, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "ctr_td3_critic_step";
    DdpgGradK gk[2] = {};
    DdpgApplyK ap[2];
    if (!critic || !net) return ddpg_fail(fn, "critic or net is NULL");
    const char *null_entry = "NULL entry in critic[2] or net[2]";
    if (!critic[0] || !critic[1] || !net[0] || !net[1]) return ddpg_fail(fn, null_entry);
    if (int r = ddpg_critics_check(fn, 2, critic, net, adam, B, workspace, workspace_bytes, null_entry,
                                   "workspace too small (ctr_td3_workspace_bytes)", gk, ap))
        return r;
    // the planes run side by side: nothing one of them writes may belong to the other
    const int nt0 = 2 * (gk[0].net.n_hidden + 1), nt1 = 2 * (gk[1].net.n_hidden + 1);
    if (ap[0].pow == ap[1].pow) return ddpg_fail(fn, "the two nets share a tensor (pow)");
    for (int t = 0; t < nt0; ++t) {
        const float *const mine[4] = {ap[0].p[t], ap[0].g[t], ap[0].m[t], ap[0].v[t]};
        for (int u = 0; u < nt1; ++u) {
            const float *const theirs[4] = {ap[1].p[u], ap[1].g[u], ap[1].m[u], ap[1].v[u]};
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j)
                    if (mine[i] == theirs[j] || mine[i] == ap[1].pow || theirs[j] == ap[0].pow)
                        return ddpg_fail(fn, "the two nets share a parameter, gradient or state tensor");
        }
    }
    if (B > 0 && (!rows || !actions || !target)) return ddpg_fail(fn, "rows, actions or target is NULL");
    if (B == 0) return 0;
    size_t shm = 0;
    for (int y = 0; y < 2; ++y)
        shm = std::max(shm, ddpg_critic_fill(gk[y], ap[y], rows, actions, scale, target, B, loss ? loss + y : nullptr));
    if (int r = allow_dynamic_lds(k_td3_grad, shm)) return r;
    const unsigned gx = grid_for(std::max(ap[0].params, ap[1].params));
    hipLaunchKernelGGL(k_td3_grad, dim3((unsigned)ap[0].slots, 2), dim3(BLOCK), shm, (hipStream_t)stream, gk[0], gk[1]);
    hipLaunchKernelGGL(k_td3_apply, dim3(gx, 2), dim3(BLOCK), 0, (hipStream_t)stream, ap[0], ap[1]);
    return hip_check("ctr_td3_critic_step launch");
}

}  // extern "C"
