// ctr_her.inc -- HER replay feed kernels + their extern "C" entry points (included at the end of
// ctr_kernels.hip, so it shares its error plumbing and launch helpers).
//
// Restates the replay side of the reference's training pipeline, stable-baselines 2 HER
// (her/replay_buffer.py HindsightExperienceReplayWrapper: add / _store_episode /
// _sample_achieved_goal; common/buffers.py ReplayBuffer.sample; her/utils.py HERGoalEnvWrapper
// convert_dict_to_obs), with the reference's settings (goal_selection_strategy 'future',
// n_sampled_goal 4: saved_policies/**/her/CTR-Generic-Reach-v0_1/CTR-Generic-Reach-v0/config.yml)
// and CtrReachEnv.compute_reward (envs/ctr_reach_env.py:160-170) for the relabelled rewards.
//
// Data layout (HBM): episode store of E = n * slots slots (slot id = env * slots + s), each
// [t_max + 1] 96-B state rows (observation + achieved goal) and [t_max] 32-B step rows (action +
// reward), env-minor ([slots][t][n], her_state_row) and written as whole dwordx4s; a slot is
// written by ONE lane (its env) while the episode runs and read by any sampler lane once closed.  Byte work only: one lane per
// env (record / open), one lane per sampled row (sample); HBM-bound gathers and scatters.
namespace {

// The sampler's prefix sums over the store's slots (her->cdf): the two launches every draw starts with.
void her_scan(const ctr_her_t *her, int64_t tiles, void *stream)
{
    hipLaunchKernelGGL(k_her_scan_tiles, dim3((unsigned)tiles), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her});
    hipLaunchKernelGGL(k_her_scan_tops, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her}, tiles);
}

int check_her(const ctr_her_t *her, const char *who)
{
    if (!her) return fail(CTR_EINVAL, who);
    const ctr_her_t &h = *her;
    if (h.n < 0 || h.n > 0x7fffffff) return fail(CTR_EINVAL, "her: n out of range");
    if (h.obs_dim != 13 && h.obs_dim != 14) return fail(CTR_EINVAL, "her: obs_dim must be 13 or 14");
    if (h.t_max < 1 || h.t_max > 65535) return fail(CTR_EINVAL, "her: t_max out of range");
    if (h.n_sampled_goal < 0 || h.n_sampled_goal > 255) return fail(CTR_EINVAL, "her: n_sampled_goal out of range");
    if (h.strategy != CTR_HER_FUTURE && h.strategy != CTR_HER_FINAL && h.strategy != CTR_HER_EPISODE)
        return fail(CTR_EINVAL, "her: unknown goal selection strategy");
    if (h.slots < 2) return fail(CTR_EINVAL, "her: slots must be >= 2");
    if (h.n > 0 && (!h.state || !h.step || !h.dg || !h.tol || !h.len || !h.epoch || !h.cur_t || !h.cur_epoch || !h.cdf))
        return fail(CTR_EINVAL, "her: buffer missing");
    if (h.n > 0 && ((reinterpret_cast<uintptr_t>(h.state) | reinterpret_cast<uintptr_t>(h.step)) & 15))
        return fail(CTR_EINVAL, "her: state / step rows must be 16-byte aligned");
    return 0;
}

}  // namespace

extern "C" {

int ctr_her_open(const ctr_her_t *her, const ctr_batch_t *batch, const float *obs, const uint8_t *mask, void *stream)
{
    if (int r = check_her(her, "ctr_her_open: her is NULL")) return r;
    if (!batch || !obs) return fail(CTR_EINVAL, "ctr_her_open: NULL argument");
    const ctr_batch_t b = *batch;
    if (b.n != her->n) return fail(CTR_EINVAL, "ctr_her_open: batch and store sizes differ");
    if (b.n == 0) return 0;
    if (!b.achieved_goal || !b.desired_goal || !b.epoch) return fail(CTR_EINVAL, "ctr_her_open: batch buffer missing");
    hipLaunchKernelGGL(k_her_open, dim3(grid_for(b.n)), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her}, b, obs, mask);
    return hip_check("ctr_her_open launch");
}

int ctr_her_record(const ctr_her_t *her, const ctr_batch_t *batch, const float *actions, const ctr_step_out_t *out,
                   double tol, void *stream)
{
    if (int r = check_her(her, "ctr_her_record: her is NULL")) return r;
    if (!batch || !out || !actions) return fail(CTR_EINVAL, "ctr_her_record: NULL argument");
    const ctr_batch_t b = *batch;
    const ctr_step_out_t o = *out;
    if (b.n != her->n) return fail(CTR_EINVAL, "ctr_her_record: batch and store sizes differ");
    if (b.n == 0) return 0;
    if (!b.achieved_goal || !b.desired_goal || !b.epoch || !b.t || !o.obs || !o.reward || !o.done ||
        !o.terminal_obs || !o.terminal_achieved)
        return fail(CTR_EINVAL, "ctr_her_record: needs the step outputs incl. terminal_obs / terminal_achieved");
    hipLaunchKernelGGL(k_her_record, dim3(grid_for(b.n)), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her}, b, actions,
                       o, tol);
    return hip_check("ctr_her_record launch");
}

int ctr_step_her(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const float *actions,
                 const ctr_step_out_t *out, int32_t autoreset, const ctr_her_t *her, void *stream)
{
    if (int r = check_her(her, "ctr_step_her: her is NULL")) return r;
    if (!batch || batch->n != her->n) return fail(CTR_EINVAL, "ctr_step_her: batch and store sizes differ");
    if (batch->n > 0 && (!batch->achieved_goal || !batch->desired_goal || !batch->epoch))
        return fail(CTR_EINVAL, "ctr_step_her: batch buffer missing");
    if (batch->env_base != her->env_base) return fail(CTR_EINVAL, "ctr_step_her: batch and store env_base differ");
    if (cfg && her->t_max != cfg->max_steps)
        return fail(CTR_EINVAL, "ctr_step_her: her->t_max must equal cfg->max_steps (episodes close at the time limit)");
    return step_launch(cfg, batch, actions, out, autoreset, her, stream);
}

int ctr_her_sample(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                   const ctr_her_batch_t *out, void *stream)
{
    if (int r = check_her(her, "ctr_her_sample: her is NULL")) return r;
    if (!out || batch_size < 0 || batch_size > 0x7fffffff) return fail(CTR_EINVAL, "ctr_her_sample: bad batch");
    if (batch_size == 0) return 0;
    if (her->n == 0) return fail(CTR_EINVAL, "ctr_her_sample: empty store");
    const ctr_her_batch_t o = *out;
    if (!o.obs || !o.action || !o.reward || !o.next_obs || !o.done) return fail(CTR_EINVAL, "ctr_her_sample: output missing");
    if ((reinterpret_cast<uintptr_t>(o.obs) | reinterpret_cast<uintptr_t>(o.next_obs) |
         reinterpret_cast<uintptr_t>(o.action)) & 15)
        return fail(CTR_EINVAL, "ctr_her_sample: obs / next_obs / action must be 16-byte aligned");
    const int64_t E = her->n * her->slots;
    const int64_t tiles = (E + HER_TILE - 1) / HER_TILE;
    if (tiles > 0x7fffffff) return fail(CTR_EINVAL, "ctr_her_sample: store too large");
    her_scan(her, tiles, stream);
    hipLaunchKernelGGL(k_her_sample, dim3(grid_for(batch_size)), dim3(BLOCK), 0, (hipStream_t)stream, HerK{*her},
                       batch_size, seed, counter, o);
    return hip_check("ctr_her_sample launch");
}

}  // extern "C"
