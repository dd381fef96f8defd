// ctr_gauss.inc -- the tanh-Gaussian policy's device pieces (include/ctr_reach_amd.h, "SAC": the
// specification): the 12-row head's layout, its logits, the noise draw and the head itself.  Included
// by ctr_kernels.hip right behind ctr_actor.inc, inside its anonymous namespace, ahead of the period
// kernels: k_collect_gauss (ctr_kernels.hip) runs them inside the period loop, k_gauss_act and
// k_her_sample_sac (ctr_sac.inc) on rows from memory.  The three kernels call these functions
// themselves, and every rounding in them is explicit under fp contract(off): that is what makes the
// three agree bit for bit.
//
// ctr_actor's MLP (actor_tile, the bf16 blob) with a 12-row output layer, rows 0..5 the mean and rows
// 6..11 the log standard deviation.  The 12 rows sit in the one 32-row output tile: rows 0..3 in
// acc[0..3] of lane half 0, rows 4..7 in acc[0..3] of lane half 1, rows 8..11 in acc[4..7] of lane
// half 0 (ctr_actor.inc's register-to-feature formula).  actor_tile adds the bias of rows 0..7;
// gauss_logits adds that of rows 8..11.

int gauss_layout(const ctr_actor_t *a, ActorK *ak)
{
    if (!a) return fail(CTR_EINVAL, "actor is NULL");
    return mlp_layout(MlpShape{"actor", 6, 12, a->in_dim, a->n_hidden, a->width}, ak);
}

// actor_check for the 12-row head: the layout, the action box and the blob.
int gauss_check(const ctr_actor_t *a, ActorK *ak)
{
    if (int r = gauss_layout(a, ak)) return r;
    for (int i = 0; i < 6; ++i) {
        if (!isfinite(a->scale[i])) return fail(CTR_EINVAL, "actor: scale must be finite");
        ak->scale[i] = a->scale[i];
    }
    return mlp_blob("actor", a->blob, ak);
}

// Six standard normals of row i of draw (seed, counter): two Philox blocks of stream 8, the
// uniforms and Box-Muller as td3_smooth makes them (ctr_critic.inc), spelled out in the same way.
__device__ __forceinline__ void gauss_eps(uint64_t seed, uint64_t counter, uint32_t i, float z[6])
{
#pragma clang fp contract(off)
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t c1 = (uint32_t)counter, c3 = (uint32_t)(counter >> 32) ^ (8u << 24);
    uint32_t w0[4] = {0u, c1, i, c3}, w1[4] = {1u, c1, i, c3};
    philox(w0, k0, k1);
    philox(w1, k0, k1);
    const float u[6] = {(float)(w0[0] >> 8) * 0x1p-24f, (float)(w0[1] >> 8) * 0x1p-24f, (float)(w0[2] >> 8) * 0x1p-24f,
                        (float)(w0[3] >> 8) * 0x1p-24f, (float)(w1[0] >> 8) * 0x1p-24f, (float)(w1[1] >> 8) * 0x1p-24f};
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float r = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, u[2 * j]))));
        float sn, cs;
        sincosf(__fmul_rn(6.2831855f, u[2 * j + 1]), &sn, &cs);
        z[2 * j] = __fmul_rn(r, cs);
        z[2 * j + 1] = __fmul_rn(r, sn);
    }
}

// max(x, 0) + log1p(exp(-|x|)): finite for every finite x
__device__ __forceinline__ float gauss_softplus(float x)
{
#pragma clang fp contract(off)
    return __fadd_rn(fmaxf(x, 0.f), log1pf(expf(-fabsf(x))));
}

// The head on one row's 12 outputs: t[i] = tanh(u_i), returns logp (the header's formulas, term by
// term, summed over i = 0..5 in that order).  det: u = the mean, eps = 0.
__device__ __forceinline__ float gauss_head(const float y[12], const float eps[6], bool det, float t[6])
{
#pragma clang fp contract(off)
    float lp = 0.f;
    #pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float s = fminf(fmaxf(y[6 + i], -20.f), 2.f);
        const float u = det ? y[i] : fmaf(expf(s), eps[i], y[i]);
        t[i] = tanhf(u);
        const float a = __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(eps[i], eps[i])), s), 0.9189385f);
        const float c = __fmul_rn(2.f, __fsub_rn(__fsub_rn(0.6931472f, u), gauss_softplus(__fmul_rn(-2.f, u))));
        lp = __fadd_rn(lp, __fsub_rn(a, c));
    }
    return lp;
}

// actor_logits for the 12-row head: the lane's row's 12 outputs, biases added.
__device__ __forceinline__ void gauss_logits(const ActorK &ak, const char *lds, const float x[20], float y[12])
{
    const int lane = (int)(threadIdx.x & 63), h = lane >> 5, r = lane & 31;
    const int lo = ak.n_hidden;                   // 1..3: the offset by constant index
    const uint32_t bo = lo == 1 ? ak.b_off[1] : (lo == 2 ? ak.b_off[2] : ak.b_off[3]);
    const float4 bb = *reinterpret_cast<const float4 *>(lds + bo + 32);      // the bias of rows 8..11
    #pragma unroll
    for (int i = 0; i < 12; ++i) y[i] = 0.f;
    #pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const actor_f32x16 acc = actor_tile<20>(ak, lds, x, c);
        const float hi[4] = {acc[4] + bb.x, acc[5] + bb.y, acc[6] + bb.z, acc[7] + bb.w};
        #pragma unroll
        for (int i = 0; i < 12; ++i) {
            const float v = __shfl(i < 8 ? acc[i & 3] : hi[i & 3], i >= 4 && i < 8 ? 32 + r : r);
            y[i] = h == c ? v : y[i];
        }
    }
}
