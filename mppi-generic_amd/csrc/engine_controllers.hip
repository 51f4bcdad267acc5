/**
 * engine_controllers.hip — mppi_compute_control (Vanilla / Colored, Tube, Robust), hand-over, getters, slide.
 * Part of the implementation of include/mppi_amd.h; see engine_internal.hpp for how the engine is divided and
 * engine_core.hip for the references its logic follows.
 */
#include "engine_internal.hpp"

/* ---------------------------------------------------------------- control loop ----------------------------------- */
mppi_status mppi_set_nominal_control(mppi_handle h, const float* u)
{
  CHECK_HANDLE(h);
  if (!u)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_set_nominal_control: null");
  std::copy(u, u + h->control_h.size(), h->control_h.begin());
  if (h->D == 2)  // Tube: both trajectories; RMPPI: nominal_control_trajectory_ = init_control_traj (:33)
    std::copy(u, u + h->control_h.size(), h->nominal_control_h.begin());
  return MPPI_OK;
}

mppi_status mppi_inject_noise(mppi_handle h, const float* eps, int n_iters)
{
  CHECK_HANDLE(h);
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (n_iters <= 0 || !eps)
  {
    h->noise_source = h->cfg.noise_source == MPPI_NOISE_INJECTED ? MPPI_NOISE_PHILOX_FUSED : h->cfg.noise_source;
    return MPPI_OK;
  }
  const size_t n = (size_t)n_iters * epsFloatsPerIteration(h);
  if (n_iters != h->n_eps_iters)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->n_eps_iters = 0;  // with the buffer: a failed allocation leaves neither
    HIP_TRY(h, h->eps_d.alloc(n));
    h->n_eps_iters = n_iters;
  }
  HIP_TRY(h, hipMemcpyAsync(h->eps_d, eps, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->noise_source = MPPI_NOISE_INJECTED;
  h->generation = 0;
  return MPPI_OK;
}

/** The one staging rule: system z's initial state, nominal control and control history go to slot z of an input block the host
 *  writes (`in`: the inbox, the pinned block).  The initial states are the system table's, x_measured where it names none; a
 *  null `mean` / `history` table leaves those slices as they are. */
static inline void stageInputs(mppi_handle h, float* in, const float* x_measured, const std::vector<float>* const mean[2],
                               const std::vector<float>* const history[2], int history_stride)
{
  for (int z = 0; z < h->D; z++)
  {
    const float* x = h->sys.x0[z] ? h->sys.x0[z]->data() : x_measured;
    std::copy(x, x + h->S, inSlice(in, h->in.x0) + z * h->S);
    if (mean)
      std::copy(mean[z]->begin(), mean[z]->end(), inSlice(in, h->in.mean) + z * h->TC);
    if (history && history[z])
      std::copy(history[z]->begin(), history[z]->end(), inSlice(in, h->in.history) + z * history_stride);
  }
}

static mppi_status uploadTube(mppi_handle h, const float* x0_actual)
{
  // both initial states and both nominal controls through the pinned input block: one copy
  stageInputs(h, h->in_pin_h, x0_actual, h->sys.control, nullptr, 0);
  const size_t n = h->in.mean.floats + 2 * (size_t)h->TC;
  HIP_TRY(h, hipMemcpyAsync(h->in_block_d, h->in_pin_h, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
  return MPPI_OK;
}

/** stats of system z from the floats the merge kernel wrote */
void parseStats(mppi_handle h, const float* st)
{
  for (int z = 0; z < h->D; z++)
  {
    const float* s = st + z * kernels::STATS_STRIDE;
    mppi_system_stats* sys = h->sys.stats[z];
    sys->baseline = s[0];
    sys->normalizer = s[1];
    sys->free_energy_mean = s[2];
    sys->free_energy_variance = s[3];
    sys->free_energy_modified_variance = s[4];
    if (s[6] != 0.0f)  // combineKernel gave up waiting for a peer's record (P2P exchange)
      h->exchange_failed = true;
  }
}

/** Host writes to the inbox (io_in_h) are complete, in order, before anything that makes the device read it.  With the BAR inbox
 *  the block is device memory behind the PCIe BAR, mapped write-combined: stores sit in the core's WC buffers until a fence (or
 *  an uncached write that happens to flush them) — every path that hands the inbox to a kernel goes through here, not only the
 *  `direct` Vanilla one (round-5 advice: the ingest launches relied on the launch path flushing the buffers).  Pinned host
 *  memory needs no fence beyond the release the doorbell write already is; one is issued anyway on non-x86 builds. */
static inline void publishInbox(mppi_handle h)
{
#if defined(__x86_64__)
  if (h->bar_inbox)
    __builtin_ia32_sfence();
#else
  (void)h;
  std::atomic_thread_fence(std::memory_order_seq_cst);
#endif
}

/** inbox -> in_block_d (one tiny kernel on the handle's stream), behind publishInbox() */
static inline void launchIngest(mppi_handle h)
{
  publishInbox(h);
  hipLaunchKernelGGL(kernels::ingestKernel, dim3(1), dim3(256), 0, h->stream, h->io_in_h.dev(), h->in_block_d, (int)h->in_floats);
}

/** spins on io_flags[idx] until reached(value); falls back to a stream synchronisation (the side stream's, and the handle's when
 *  `sync_stream`) when the flag does not show within the limit (a failed launch, a wedged device): the caller then sees the HIP
 *  error, or `what`, instead of a hang */
template <class Reached>
static inline mppi_status spinOnFlag(mppi_handle h, int idx, Reached reached, bool sync_stream, const char* what)
{
  using clock = std::chrono::steady_clock;
  const clock::time_point t0 = clock::now();
  volatile unsigned* flag = h->io_flags_h + idx;
  unsigned spins = 0;
  while (!reached(__atomic_load_n(flag, __ATOMIC_ACQUIRE)))
  {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
    if ((++spins & 0x3ff) == 0 && std::chrono::duration<double>(clock::now() - t0).count() > 2.0)
    {
      if (sync_stream)
        HIP_TRY(h, hipStreamSynchronize(h->stream));
      if (h->side_stream)
        HIP_TRY(h, hipStreamSynchronize(h->side_stream));
      if (!reached(__atomic_load_n(flag, __ATOMIC_ACQUIRE)))
        return fail(h, MPPI_ERR_HIP, what);
      break;
    }
  }
  return MPPI_OK;
}

/** a flag the finalize kernel (or raiseFlagKernel) raises in host memory shows hand-over `seq` */
static mppi_status waitHostFlag(mppi_handle h, int idx, unsigned seq)
{
  return spinOnFlag(h, idx, [seq](unsigned v) { return v == seq; }, true,
                    "the finalize kernel finished without raising its hand-over flag");
}

/** the flag has reached seq (sequence numbers only grow; wrap-around safe): the trajectory phases of a split hand-over run in
 *  order on the side stream, so a later call's flag value covers the earlier ones */
static mppi_status waitHostFlagReached(mppi_handle h, int idx, unsigned seq)
{
  return spinOnFlag(h, idx, [seq](unsigned v) { return (int)(v - seq) >= 0; }, false,
                    "the trajectory phase of an earlier call finished without raising its flag");
}

/** everything enqueued on the handle's stream so far is done: a flag raised behind it that the host spins on (`counter`: the
 *  flag's own hand-over count), or — MPPI_AMD_NO_SPIN=1 — a stream synchronisation */
static mppi_status streamRoundTrip(mppi_handle h, int idx, unsigned& counter)
{
  if (!h->low_latency)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
  }
  const unsigned seq = ++counter;
  hipLaunchKernelGGL(kernels::raiseFlagKernel, dim3(1), dim3(64), 0, h->stream, h->io_flags_h.dev() + idx, seq);
  HIP_TRY(h, hipGetLastError());
  return waitHostFlag(h, idx, seq);
}

/** the state / output trajectories of the last low-latency computeControl: wait for the finalize kernel's second flag of every
 *  system, then take the state sequences through the system table */
static mppi_status ensureTrajectories(mppi_handle h)
{
  if (!h->traj_pending)
    return MPPI_OK;
  MPPI_TRY(waitHostFlag(h, 1, h->io_seq));
  if (h->D == 2)
    MPPI_TRY(waitHostFlag(h, 3, h->io_seq));
  h->traj_pending = false;
  const size_t n = (size_t)h->cfg.num_timesteps * h->S;
  const float* xs = outSlice(h->io_out_h, h->out.state);
  for (int z = 0; z < h->D; z++)
    std::copy(xs + z * n, xs + (z + 1) * n, h->sys.state[z]->begin());
  // base_plant.hpp:515-528 checks the state trajectory as well as the control.  Robust: the nominal trajectory only (system 0:
  // the next call's candidates start from it); Tube: both (the nominal one's first state is where the next call starts from)
  if (h->cfg.controller == MPPI_CONTROLLER_ROBUST && !allFinite(h->nominal_state_h))
    return fail(h, MPPI_ERR_NAN, "non-finite value in the nominal state sequence of the last mppi_compute_control");
  if (h->cfg.controller == MPPI_CONTROLLER_TUBE && (!allFinite(h->state_h) || !allFinite(h->nominal_state_h)))
    return fail(h, MPPI_ERR_NAN, "non-finite value in the state sequences of the last mppi_compute_control");
  if (h->D == 1 && !allFinite(h->state_h))
    return fail(h, MPPI_ERR_NAN, "non-finite value in the state sequence of the last mppi_compute_control");
  return MPPI_OK;
}

/** points a finalize pass at the device-mapped outbox and takes the next hand-over sequence number; stats_systems: how many
 *  systems' merge statistics travel with the control sequences (0: a pass that only re-rolls a trajectory) */
static inline void toOutbox(mppi_handle h, kernels::FinalizeArgs& a, int stats_systems)
{
  float* out = h->io_out_h.dev();
  a.control_out_d = outSlice(out, h->out.control);
  a.state_out_d = outSlice(out, h->out.state);
  a.output_out_d = outSlice(out, h->out.output);
  if (stats_systems > 0)
  {
    a.stats_in_d = h->stats_d;
    a.stats_out_d = outSlice(out, h->out.stats);
    a.stats_floats = stats_systems * kernels::STATS_STRIDE;
  }
  a.flags_d = h->io_flags_h.dev();
  a.seq = ++h->io_seq;
}

/** Launches the finalize pass `a` (pointed at the outbox) for num_systems systems and marks the outbox as holding the results.
 *  One launch — or, split hand-over (mppi_handle_s::split_finalize), two.  The control phase runs on the handle's stream, as
 *  kernels::mergeControlKernel when `merge` brings the last rollout launch's un-merged records along; it leaves a copy of the
 *  input block carry_src_d in this call's carry block.  The trajectory phase runs on the side stream: it waits for the carry block
 *  by itself (no event between the streams) and reads nothing else.  a.carry_d is that block afterwards. */
static mppi_status launchHandover(mppi_handle h, kernels::FinalizeArgs& a, int num_systems, const float* carry_src_d,
                                  const kernels::MergeControlArgs* merge)
{
  std::string err;
  if (h->split_finalize)
  {
    // this call's carry block was last read by the trajectory phase of the call two hand-overs ago: its flags are up, or we wait
    const unsigned p = a.seq & 1u;
    if (h->carry_seq[p] != 0)
      for (int z = 0; z < num_systems; z++)
        MPPI_TRY(waitHostFlagReached(h, 2 * z + 1, h->carry_seq[p]));
    a.phases = 1;
    a.carry_d = h->carry_d + (size_t)p * h->in_floats;
    a.carry_src_d = carry_src_d;
    a.carry_floats = (int)h->in_floats;
    a.carry_mean_off = (int)h->in.mean.floats;
    a.carry_ready_d = reinterpret_cast<unsigned*>(h->carry_d + 2 * h->in_floats) + 2 * p;
  }
  const mppi_status st = merge ? h->model->launchMergeControl(a, *merge, h->stream, err) :
                                 h->model->launchFinalize(num_systems, a, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  if (h->split_finalize)
  {
    kernels::FinalizeArgs b = a;
    b.phases = 2;
    b.carry_d = nullptr;
    b.control_in_d = inSlice(a.carry_d, h->in.mean);
    b.x0_d = inSlice(a.carry_d, h->in.x0);
    b.smooth_mask = 0;
    b.scratch_d = h->fin_scratch2_d;
    const mppi_status st2 = h->model->launchFinalize(num_systems, b, h->side_stream, err);
    if (st2 != MPPI_OK)
      return fail(h, st2, err);
    HIP_TRY(h, hipEventRecord(h->ev_side, h->side_stream));
    h->side_pending = true;
    h->carry_seq[a.seq & 1u] = a.seq;
  }
  h->out_pin_fresh = false;
  h->results_in_io = true;
  h->traj_pending = true;  // set before the waits: a failing wait must not leave io_out unguarded for the next call
  return MPPI_OK;
}

/** The control sequences and the merge statistics of hand-over io_seq are out (flag 0, and flag 2 of a second system): take
 *  them through the system table.  after_wait(): what the caller does between the waits and the copies (Vanilla's host stamp). */
template <class AfterWait>
static inline mppi_status takeControls(mppi_handle h, AfterWait after_wait)
{
  for (int z = 0; z < h->D; z++)
    MPPI_TRY(waitHostFlag(h, 2 * z, h->io_seq));
  after_wait();
  const float* u = outSlice(h->io_out_h, h->out.control);
  for (int z = 0; z < h->D; z++)
    std::copy(u + (size_t)z * h->TC, u + (size_t)(z + 1) * h->TC, h->sys.control[z]->begin());
  parseStats(h, outSlice(h->io_out_h, h->out.stats));
  h->stats_h_fresh = true;
  return MPPI_OK;
}

/** Nothing has weight: every trajectory cost of system z was +inf (or NaN) in the last merge — the baseline is not finite, or the
 *  normaliser is not a positive finite number — and u* is NaN.  The Vanilla control phase clamps u* to the control ranges with
 *  fminf(fmaxf(lo, u), hi) (the reference's enforceConstraints), which DROPS a NaN: with the default ranges the control handed
 *  back is -FLT_MAX in every entry and passes a finiteness check.  Read from the statistics that travel with the control. */
static inline bool nothingHasWeight(mppi_handle h, int z)
{
  const mppi_system_stats* s = h->sys.stats[z];
  return !std::isfinite(s->baseline) || !std::isfinite(s->normalizer) || !(s->normalizer > 0.0f);
}

/** reference: controllers/MPPI/mppi_controller.cu:152-231; ColoredMPPI/colored_mppi_controller.cu:150-237 */
static mppi_status computeControlVanilla(mppi_handle h, const float* x0_true, int stride)
{
  const int T = h->cfg.num_timesteps;
  h->pending_records_d = nullptr;  // this call uploads its own mean: nothing of an earlier (failed) call may be merged over it
  PendingRecordsGuard guard{ h };
  // ColoredMPPI state leash (colored_mppi_controller.cu:150-156): the optimisation starts from the state of the previous
  // solution at index leash_jump, pulled towards the measured state by at most the leash per dimension
  std::vector<float> leashed;
  const float* x0 = x0_true;
  if (h->cfg.controller == MPPI_CONTROLLER_COLORED && h->leash_active)
  {
    MPPI_TRY(ensureTrajectories(h));
    leashed.resize(h->S);
    h->model->hostEnforceLeash(x0_true, &h->state_h[(size_t)h->leash_jump * h->S], h->leash_dist.data(), leashed.data());
    x0 = leashed.data();
  }
  kernels::FinalizeArgs a = finalizeArgs(h, h->mean_d, 0, /*smooth*/ 1, /*constrain*/ 1);
  if (h->low_latency)
  {
    /* Inputs and results travel through host memory mapped into the device: no copy command, no stream synchronisation.
     * The call returns when the control sequence and the merge statistics are out (flag 0), while the finalize kernel
     * still re-rolls the state trajectory of u* — a T-step serial chain, ~1/3 of the call for Cartpole; the trajectory
     * getters wait for flag 1 (tools/ubench/handover.hip: 3 kernels + spin 15 us against 23 us with copies + synchronise). */
    // a caller that never asked for the previous trajectories: the kernel must be done with io_out and — BAR inbox — with the
    // inputs before the host overwrites them.  Split hand-over: the trajectory phase reads its carry block, writes nothing the
    // control phase of this call writes, and the flag waits of the getters take sequence numbers: nothing to wait for
    if (h->traj_pending && !h->split_finalize)
      MPPI_TRY(waitHostFlag(h, 1, h->io_seq));
    h->traj_pending = false;
    const std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    auto stamp = [&](int i) {
      h->host_stamps_us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count();
    };
    stageInputs(h, h->io_in_h, x0, h->sys.control, h->sys.history, 0);
    stamp(0);
    // BAR inbox: no ingest launch — the kernels of this call read the inbox (device memory the stores above went to) themselves
    const bool direct = h->bar_inbox && h->cfg.num_iters >= 1 && h->reduction_mode == MPPI_REDUCTION_FUSED && !tsallisActive(h) &&
                        !exchangeActive(h);
    struct SourceGuard  // the overrides never outlive the call
    {
      mppi_handle h;
      ~SourceGuard()
      {
        h->x0_src_d = h->mean_src_d = nullptr;
      }
    } source_guard{ h };
    if (direct)
    {
      publishInbox(h);  // the write-combined stores are out before the doorbell of the first launch
      h->x0_src_d = inSlice(h->io_in_h.dev(), h->in.x0);
      h->mean_src_d = inSlice(h->io_in_h.dev(), h->in.mean);
      a.x0_d = h->x0_src_d;
      a.history_d = inSlice(h->io_in_h.dev(), h->in.history);
    }
    else
    {
      launchIngest(h);
      HIP_TRY(h, hipGetLastError());
    }
    stamp(1);
    for (int it = 0; it < h->cfg.num_iters; it++)
      MPPI_TRY(iteration(h, it, stride));
    stamp(2);
    // The last iteration's records (streamed merge) are still un-merged.  Split hand-over on a model with the plain one-wave
    // finalize form: the control phase merges them itself (kernels::mergeControlKernel) — one launch on the call's critical
    // path where combineKernel + control phase were two.  Otherwise: merge now; everything below reads mean_d / stats_d.
    const float* fuse_records = nullptr;
    if (h->pending_records_d && h->split_finalize && h->merge_control_enabled && !a.scratch_d && streamMergeApplies(h) &&
        h->model->supportsMergeControl(T))
    {
      fuse_records = h->pending_records_d;
      h->pending_records_d = nullptr;
    }
    else
      MPPI_TRY(flushMerge(h));
    stamp(3);
    toOutbox(h, a, 1);
    // (x0 and the control history: the slices on either side of the mean)
    auto ingest_ranges = [&](const float* src) -> mppi_status {
      hipLaunchKernelGGL(kernels::ingestRangesKernel, dim3(1), dim3(256), 0, h->stream, src, h->in_block_d,
                         (int)h->in.mean.floats, (int)h->in.history.floats, (int)(h->in_floats - h->in.history.floats));
      HIP_TRY(h, hipGetLastError());
      return MPPI_OK;
    };
    // Single-launch hand-over with the BAR inbox (MPPI_AMD_SPLIT_FINALIZE=0): the device-resident copy of x0 / history is taken
    // from the INBOX, so it has to be taken before the finalize kernel raises flag 1 — the next call waits for nothing else
    // before it rewrites the inbox (round-5 advice: behind the finalize kernel the copy could read a half-rewritten inbox).  It
    // touches neither what the finalize kernel reads (inbox, mean_d) nor what it writes.
    if (direct && !h->split_finalize)
      MPPI_TRY(ingest_ranges(h->io_in_h.dev()));
    kernels::MergeControlArgs m{};
    if (fuse_records)
    {
      m.records_t_d = recordsTransposed(h, const_cast<float*>(fuse_records));
      m.num_records = h->num_blocks;
      m.lambda = h->cfg.lambda;
      m.num_rollouts_total = h->cfg.num_rollouts;
      m.mean_out_d = h->mean_d;
      m.stats_d = h->stats_d;
      h->n_merge_launches++;  // (the merge of this call: inside the control phase's launch)
    }
    MPPI_TRY(launchHandover(h, a, 1, direct ? h->io_in_h.dev() : h->in_block_d, fuse_records ? &m : nullptr));
    if (direct && h->split_finalize)
    {  // behind the control phase, off the caller's path: the device-resident x0 / history later mppi_optimize / operator calls
       // read — from the CARRY block (the host may be rewriting the inbox for its next call by now; the carry block of this parity
       // is not rewritten before the call after next, which first waits for this call's flag 1)
      MPPI_TRY(ingest_ranges(a.carry_d));
    }
    stamp(4);
    MPPI_TRY(takeControls(h, [&] { stamp(5); }));
    stamp(6);
    if (!allFinite(h->control_h))
      return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite value in the control sequence");
    if (h->cfg.num_iters >= 1 && nothingHasWeight(h, 0))
      return fail(h, MPPI_ERR_NAN, "mppi_compute_control: no rollout has weight (every trajectory cost is non-finite)");
    return MPPI_OK;
  }
  // one hand-over in (x0, nominal control, control history), one back (control, state and output trajectories, stats):
  // two copies through pinned memory and a single synchronisation per call
  stageInputs(h, h->in_pin_h, x0, h->sys.control, h->sys.history, 0);
  HIP_TRY(h, hipMemcpyAsync(h->in_block_d, h->in_pin_h, sizeof(float) * h->in_floats, hipMemcpyHostToDevice, h->stream));
  for (int it = 0; it < h->cfg.num_iters; it++)
    MPPI_TRY(iteration(h, it, stride));
  MPPI_TRY(flushMerge(h));  // the last iteration's records (streamed merge): everything below reads mean_d / stats_d
  std::string err;
  const mppi_status st = h->model->launchFinalize(1, a, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  HIP_TRY(h, hipMemcpyAsync(h->out_pin_h, h->out_block_d, sizeof(float) * h->out_floats, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const float* u = outSlice(h->out_pin_h, h->out.control);
  const float* xs = outSlice(h->out_pin_h, h->out.state);
  std::copy(u, u + (size_t)T * h->C, h->control_h.begin());
  std::copy(xs, xs + (size_t)T * h->S, h->state_h.begin());
  parseStats(h, outSlice(h->out_pin_h, h->out.stats));
  h->out_pin_fresh = true;
  h->results_in_io = false;
  // base_plant.hpp:515-528 checks both the control and the state trajectory
  if (!allFinite(h->control_h) || !allFinite(h->state_h))
    return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite value in the control or state sequence");
  if (h->cfg.num_iters >= 1 && nothingHasWeight(h, 0))
    return fail(h, MPPI_ERR_NAN, "mppi_compute_control: no rollout has weight (every trajectory cost is non-finite)");
  return MPPI_OK;
}

/** reference: Tube-MPPI/tube_mppi_controller.cu:157-299 */
static mppi_status computeControlTube(mppi_handle h, const float* x0, int stride)
{
  const int S = h->S;
  if (!h->nominal_state_init)
  {
    std::copy(x0, x0 + S, h->nominal_state_h.begin());
    std::copy(x0, x0 + S, h->tube_x_h.begin());
    h->nominal_state_init = true;
  }
  if (h->low_latency)
  {
    /* Inputs and results through host memory mapped into the device, flags instead of copies + synchronisations (see
     * computeControlVanilla): the call returns with both control sequences and leaves the two trajectories to
     * ensureTrajectories(). */
    // (split hand-over: nothing of this call touches what the last call's trajectory phase reads or writes — see
    // computeControlVanilla — and the nominal system's state is tube_x_h, not row 0 of a trajectory still on its way)
    if (!h->split_finalize)
      MPPI_TRY(ensureTrajectories(h));
    /* Round 5: ONE hand-over per call.  Between two optimisation passes the reference decides on the host whether the nominal
     * system restarts from the actual one (:264-277) — after computing both state trajectories, of which the decision needs
     * nothing and the next pass only row 0, the initial state.  Rounds 2-4 mirrored that: finalize pass, wait for both
     * trajectories, decide, stage, second finalize pass (control on the host after 86 us at config 3).  The decision is two
     * baselines the merge has just written: tubeSelectKernel takes it on the device (nominal mean and initial state
     * overwritten where the actual system wins), the passes chain without the host, and a single finalize pass — smoothing the
     * nominal control, re-rolling both trajectories — hands everything over.  Same values in every host-visible field. */
    stageInputs(h, h->io_in_h, x0, h->sys.control, h->sys.history, 0);
    launchIngest(h);
    HIP_TRY(h, hipGetLastError());
    for (int it = 0; it < h->cfg.num_iters; it++)
    {
      MPPI_TRY(iteration(h, it, stride));
      hipLaunchKernelGGL(kernels::tubeSelectKernel, dim3(1), dim3(256), 0, h->stream, h->stats_d, h->mean_d, h->x0_d, h->TC, S,
                         h->nominal_threshold);
      HIP_TRY(h, hipGetLastError());
    }
    // smoothControlTrajectory() smooths the nominal control (:281, :325-329), then computeStateTrajectory(state).  Split hand-over
    // as in computeControlVanilla: both systems' re-rollouts on the side stream, from the carry block — a copy of the ingested
    // input block, where tubeSelectKernel has put the chosen nominal state and control
    kernels::FinalizeArgs a = finalizeArgs(h, h->mean_d, 0, /*smooth nominal*/ 2, 0);
    toOutbox(h, a, 2);
    MPPI_TRY(launchHandover(h, a, 2, h->in_block_d, nullptr));
    MPPI_TRY(takeControls(h, [] {}));
    if (h->cfg.num_iters > 0)
    {
      const float* st1 = outSlice(h->io_out_h, h->out.stats) + kernels::STATS_STRIDE;
      // tubeSelectKernel: bit 0 = the LAST pass kept the nominal system (nominalStateUsed), bit 1 = the nominal system's initial
      // state on the device is the actual one — after a take-over in ANY pass of this call (the reference's
      // nominal_state_trajectory_ persists across the passes, tube_mppi_controller.cu:268-277), not only in the last
      const int sel = (int)st1[7];
      h->stats_h.nominal_state_used = sel & 1;
      if (sel & 2)
        std::copy(x0, x0 + S, h->tube_x_h.begin());
    }
    if (!allFinite(h->control_h) || !allFinite(h->nominal_control_h))
      return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite value in the control sequence");
    return MPPI_OK;
  }
  for (int it = 0; it < h->cfg.num_iters; it++)
  {
    MPPI_TRY(uploadTube(h, x0));
    MPPI_TRY(iteration(h, it, stride));
    // new means -> host control_ / nominal_control_trajectory_, then both state trajectories (:255-263)
    MPPI_TRY(finalize(h, h->mean_d, 0, 0, h->sys.control, h->sys.state));
    MPPI_TRY(fetchStats(h));
    if (h->stats_h.real_sys.baseline < h->stats_h.nominal_sys.baseline + h->nominal_threshold)
    {
      h->stats_h.nominal_state_used = 0;
      h->nominal_state_h = h->state_h;
      std::copy(x0, x0 + S, h->tube_x_h.begin());
      h->nominal_control_h = h->control_h;
    }
    else
    {
      h->stats_h.nominal_state_used = 1;
    }
  }
  // smoothControlTrajectory() smooths the nominal control (:281, :325-329), then computeStateTrajectory(state)
  HIP_TRY(h, hipMemcpyAsync(h->ctrl_in_d, h->control_h.data(), sizeof(float) * h->TC, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->ctrl_in_d + h->TC, h->nominal_control_h.data(), sizeof(float) * h->TC,
                            hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->x0_d + S, h->tube_x_h.data(), sizeof(float) * S, hipMemcpyHostToDevice, h->stream));
  MPPI_TRY(finalize(h, h->ctrl_in_d, /*smooth nominal*/ 2, 0, h->sys.control, h->sys.state));
  if (!allFinite(h->control_h) || !allFinite(h->nominal_control_h) || !allFinite(h->state_h) ||
      !allFinite(h->nominal_state_h))
    return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite value in the control or state sequence");
  return MPPI_OK;
}


/* ---------------------------------------------------------------- Robust MPPI host logic ------------------------- */
/** reference: robust_mppi_controller.cu:480-500 (computeLineSearchWeights) — [3][NC] row-major */
static void rmLineSearchWeights(int nc, std::vector<float>& w)
{
  w.assign((size_t)3 * nc, 0.0f);
  const int half = nc / 2;
  for (int i = 0; i < half + 1; i++)
  {
    w[0 * nc + i] = 1 - i / float(half);
    w[1 * nc + i] = i / float(half);
    w[2 * nc + i] = 0.0f;
  }
  for (int i = 1; i < half + 1; i++)
  {
    w[0 * nc + half + i] = 0.0f;
    w[1 * nc + half + i] = 1 - i / float(half);
    w[2 * nc + half + i] = i / float(half);
  }
}
/** reference: robust_mppi_controller.cu:502-512 — round((0, stride, stride) . weights) */
static void rmImportanceSamplerStrides(int stride, int nc, const std::vector<float>& w, std::vector<int>& out)
{
  out.resize(nc);
  for (int i = 0; i < nc; i++)
  {
    float acc = 0.0f * w[0 * nc + i];
    acc += (float)stride * w[1 * nc + i];
    acc += (float)stride * w[2 * nc + i];
    out[i] = (int)roundf(acc);
  }
}
/** reference: robust_mppi_controller.cu:514-545 (computeCandidateBaseline, computeBestIndex); expf / logf -> det */
static void rmBestIndex(mppi_handle h)
{
  const int nc = h->num_candidates, ns = h->samples_per_candidate;
  const float lambda = h->cfg.lambda;
  float baseline = h->rm_cand_costs[0];
  for (int i = 1; i < nc * ns; i++)
    if (h->rm_cand_costs[i] < baseline)
      baseline = h->rm_cand_costs[i];
  h->rm_cand_free_energy.assign(nc, 0.0f);
  for (int i = 0; i < nc; i++)
  {
    float fe = 0.0f;
    for (int j = 0; j < ns; j++)
      fe += mppi::det::exp((float)(-1.0 / (double)lambda * (double)(h->rm_cand_costs[(size_t)i * ns + j] - baseline)));
    fe = (float)((double)fe / (1.0 * ns));
    fe = -lambda * mppi::det::log(fe) + baseline;
    h->rm_cand_free_energy[i] = fe;
    if (fe < h->value_function_threshold)
      h->best_index = i;
  }
}

static mppi_status rmEnsureCandidateBuffers(mppi_handle h)
{
  const int n = h->num_candidates * h->samples_per_candidate;
  if ((size_t)n <= h->cand_costs_d.size() && (size_t)h->num_candidates <= h->cand_strides_d.size())
    return MPPI_OK;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->cand_states_d.reset();
  h->cand_costs_d.reset();
  h->cand_strides_d.reset();
  HIP_TRY(h, h->cand_io_h.allocHost((size_t)h->num_candidates * (h->S + 1) + n, hipHostMallocMapped | hipHostMallocCoherent));
  HIP_TRY(h, h->cand_states_d.alloc((size_t)h->num_candidates * h->S));
  HIP_TRY(h, h->cand_costs_d.alloc(n));
  HIP_TRY(h, h->cand_strides_d.alloc(h->num_candidates));
  return MPPI_OK;
}

/** the nominal state trajectory from rm_nominal_state under nominal_control_h (computeStateTrajectoryHelper) */
static mppi_status rmNominalStateTrajectory(mppi_handle h)
{
  if (h->low_latency)
  {
    // inputs with the input block, the trajectory back through the device-mapped output block + flag (system 0 only)
    std::copy(h->rm_nominal_state.begin(), h->rm_nominal_state.end(), inSlice(h->io_in_h, h->in.x0));
    std::copy(h->nominal_control_h.begin(), h->nominal_control_h.end(), inSlice(h->io_in_h, h->in.mean));
    launchIngest(h);
    HIP_TRY(h, hipGetLastError());
    kernels::FinalizeArgs a = finalizeArgs(h, h->mean_d, 0, 0, 0);
    toOutbox(h, a, /*no statistics*/ 0);
    std::string err;
    const mppi_status st = h->model->launchFinalize(1, a, h->stream, err);
    if (st != MPPI_OK)
      return fail(h, st, err);
    h->out_pin_fresh = false;
    h->results_in_io = true;
    MPPI_TRY(waitHostFlag(h, 1, h->io_seq));
    const float* xs = outSlice(h->io_out_h, h->out.state);
    std::copy(xs, xs + h->nominal_state_h.size(), h->nominal_state_h.begin());
    return MPPI_OK;
  }
  HIP_TRY(h, hipMemcpyAsync(h->x0_d, h->rm_nominal_state.data(), sizeof(float) * h->S, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->ctrl_in_d, h->nominal_control_h.data(), sizeof(float) * h->TC, hipMemcpyHostToDevice,
                            h->stream));
  return finalize(h, h->ctrl_in_d, 0, 0, nullptr, h->sys.state, /*the nominal system alone*/ 1);
}

/** reference: robust_mppi_controller.cu:571-626 (computeNominalStateAndStride) */
static mppi_status rmNominalStateAndStride(mppi_handle h, const float* state, int stride)
{
  const int S = h->S, nc = h->num_candidates, ns = h->samples_per_candidate;
  if (!h->rm_nominal_init)
  {
    std::copy(state, state + S, h->rm_nominal_state.begin());
    h->rm_nominal_init = true;
    h->nominal_stride = 0;
    return MPPI_OK;
  }
  // (injected noise on a K-sharded handle: the slab this call consumes must hold the GLOBAL rollouts' rows 0 .. ns-1 on
  //  every rank — the evaluation samples are the same rows for every candidate and every rank, robust_mppi_controller.cu:596)
  if (ns > h->K_local && h->noise_source == MPPI_NOISE_INJECTED)
    return fail(h, MPPI_ERR_INVALID_ARG, "samples_per_candidate exceeds the injected noise rows");
  // candidates = [nominal_x_k, nominal_x_k+1, real_x_k+1] * line search weights (:350-362)
  rmLineSearchWeights(nc, h->rm_line_weights);
  h->rm_cand_states.assign((size_t)nc * S, 0.0f);
  for (int c = 0; c < nc; c++)
    for (int i = 0; i < S; i++)
    {
      float acc = h->nominal_state_h[0 * S + i] * h->rm_line_weights[0 * nc + c];
      acc += h->nominal_state_h[1 * S + i] * h->rm_line_weights[1 * nc + c];
      acc += state[i] * h->rm_line_weights[2 * nc + c];
      h->rm_cand_states[(size_t)c * S + i] = acc;
    }
  rmImportanceSamplerStrides(stride, nc, h->rm_line_weights, h->rm_cand_strides);
  MPPI_TRY(rmEnsureCandidateBuffers(h));
  float* cand_costs_dev = h->cand_costs_d;
  if (h->low_latency)
  {
    // candidate states and strides stay in host memory mapped into the device (the kernel reads them once, in place), the
    // nominal control goes up with the input block: no copy command
    std::copy(h->rm_cand_states.begin(), h->rm_cand_states.end(), h->cand_io_h.get());
    std::memcpy(h->cand_io_h + (size_t)nc * S, h->rm_cand_strides.data(), sizeof(int) * nc);
    std::copy(h->nominal_control_h.begin(), h->nominal_control_h.end(), inSlice(h->io_in_h, h->in.mean));
    launchIngest(h);
    HIP_TRY(h, hipGetLastError());
    cand_costs_dev = h->cand_io_h.dev() + (size_t)nc * (S + 1);
  }
  else
  {
    HIP_TRY(h, hipMemcpyAsync(h->cand_states_d, h->rm_cand_states.data(), sizeof(float) * nc * S, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->cand_strides_d, h->rm_cand_strides.data(), sizeof(int) * nc, hipMemcpyHostToDevice,
                              h->stream));
    // copyNominalControlToDevice: distribution 0 <- nominal control (:409-412)
    HIP_TRY(h, hipMemcpyAsync(h->mean_d, h->nominal_control_h.data(), sizeof(float) * h->TC, hipMemcpyHostToDevice,
                              h->stream));
  }
  /* K-sharded handles connected over the P2P mailbox evaluate the candidates SHARDED BY CANDIDATE ("RMPPI
   * init-eval shards over candidates x samples the same way"): rank r takes candidates [r * ceil(nc / world), ...), writes
   * their costs at their position of the array in every peer's aux mailbox (postAuxKernel) and every rank assembles all
   * nc x ns costs from its own (gatherAuxKernel) — same kernel, same bits as the replicated evaluation, 1 / world of the work.
   * Other exchanges (RCCL, caller-driven) keep evaluating all candidates on every rank: the costs are needed on the HOST of
   * every rank, and a block's T-step chain takes as long for one candidate as for nine. */
  const int world = h->cfg.world_size;
  const bool shard_eval = world > 1 && h->p2p_ready && nc * ns <= kernels::MAILBOX_AUX_FLOATS;
  int c_lo = 0, c_hi = nc;
  if (shard_eval)
  {
    const int chunk = (nc + world - 1) / world;
    c_lo = std::min(nc, h->cfg.rank * chunk);
    c_hi = std::min(nc, c_lo + chunk);
  }
  kernels::InitEvalArgs a{};
  a.dt = h->cfg.dt;
  a.num_timesteps = h->cfg.num_timesteps;
  a.num_eval_rollouts = (c_hi - c_lo) * ns;
  a.samples_per_candidate = ns;
  a.lambda = h->cfg.lambda;
  a.alpha = h->cfg.alpha;
  a.strides_d = (h->low_latency ? reinterpret_cast<const int*>(h->cand_io_h.dev() + (size_t)nc * S) : h->cand_strides_d) + c_lo;
  a.states_d = (h->low_latency ? h->cand_io_h.dev() : h->cand_states_d) + (size_t)c_lo * S;
  // sharded: the slice goes to the device buffer (posted from there), the assembled array to where the host reads it
  float* slice_dev = (shard_eval ? h->cand_costs_d : cand_costs_dev) + (size_t)c_lo * ns;
  a.trajectory_costs_d = slice_dev;
  SamplerLaunchState s{};
  s.num_rollouts_local = h->K_local;
  s.num_rollouts_global = h->cfg.num_rollouts;
  s.rollout_offset = 0;  // eval samples are the GLOBAL rollouts 0 .. samples_per_candidate-1 on every rank
  s.num_timesteps = h->cfg.num_timesteps;
  s.num_distributions = h->D;
  s.control_means_d = h->mean_d;
  s.eps_d = nullptr;
  if (h->noise_source == MPPI_NOISE_INJECTED)
  {
    if (!h->eps_d || h->n_eps_iters <= 0)
      return fail(h, MPPI_ERR_STATE, "noise source is MPPI_NOISE_INJECTED but no noise has been injected");
    s.eps_d = h->eps_d + (size_t)(h->generation % (uint32_t)h->n_eps_iters) * epsFloatsPerIteration(h);
  }
  else if (h->noise_source == MPPI_NOISE_ROCRAND_HOST)
    return fail(h, MPPI_ERR_UNSUPPORTED, "this call draws through the sampler's random-access path: use the Philox or the "
                                         "injected noise source (MPPI_NOISE_ROCRAND_HOST fills the rollout kernel's eps buffer only)");
  s.control_samples_d = nullptr;
  s.seed = h->cfg.seed;
  s.generation = h->generation;
  s.iteration = 0;  // generateSamples(stride, 0, gen) (:596)
  s.optimization_stride = stride;
  s.independent_noise = h->independent_noise ? 1 : 0;
  std::string err;
  if (c_hi > c_lo)
  {
    mppi_status st = h->model->launchInitEval(h->rm_pipeline, a, s, h->stream, err);
    if (st != MPPI_OK)
      return fail(h, st, err);
  }
  h->generation++;
  if (shard_eval)
  {
    const unsigned seq = ++h->aseq;
    const unsigned parity = seq & 1u;
    kernels::AuxTargets t{};
    t.world = world;
    t.seq = seq;
    for (int p = 0; p < world; p++)
    {
      float* aux = h->peer_mbox[p] + h->mbox_aux_off;
      t.peer_aux[p] = aux + (size_t)parity * kernels::MAILBOX_AUX_FLOATS;
      t.peer_flag[p] = reinterpret_cast<unsigned*>(aux + 2 * (size_t)kernels::MAILBOX_AUX_FLOATS) + parity * world + h->cfg.rank;
    }
    hipLaunchKernelGGL(kernels::postAuxKernel, dim3(1), dim3(256), 0, h->stream, slice_dev, c_lo * ns, (c_hi - c_lo) * ns, t);
    const float* my_aux = h->mbox_d + h->mbox_aux_off;
    hipLaunchKernelGGL(kernels::gatherAuxKernel, dim3(1), dim3(256), 0, h->stream,
                       my_aux + (size_t)parity * kernels::MAILBOX_AUX_FLOATS,
                       reinterpret_cast<const unsigned*>(my_aux + 2 * (size_t)kernels::MAILBOX_AUX_FLOATS) + parity * world, world,
                       seq, 200000000ull, nc * ns, cand_costs_dev);
    HIP_TRY(h, hipGetLastError());
  }
  h->rm_cand_costs.resize((size_t)nc * ns);
  if (!h->low_latency)
    HIP_TRY(h, hipMemcpyAsync(h->rm_cand_costs.data(), h->cand_costs_d, sizeof(float) * nc * ns, hipMemcpyDeviceToHost,
                              h->stream));
  MPPI_TRY(streamRoundTrip(h, 9, h->cand_seq));
  if (h->low_latency)
  {  // (the kernel wrote them in place)
    const float* costs = h->cand_io_h + (size_t)nc * (S + 1);
    std::copy(costs, costs + (size_t)nc * ns, h->rm_cand_costs.begin());
  }
  if (shard_eval)
    for (float c : h->rm_cand_costs)
      if (c != c)  // gatherAuxKernel's mark: a peer never delivered its slice (a trajectory cost itself is clamped, never NaN)
        return fail(h, MPPI_ERR_COMM, "Robust MPPI candidate evaluation: a peer's slice of the candidate costs did not arrive");
  rmBestIndex(h);
  h->stats_h.nominal_state_used = h->best_index;
  h->nominal_stride = h->rm_cand_strides[h->best_index];
  std::copy(h->rm_cand_states.begin() + (size_t)h->best_index * S, h->rm_cand_states.begin() + (size_t)(h->best_index + 1) * S,
            h->rm_nominal_state.begin());
  return MPPI_OK;
}

/** reference: robust_mppi_controller.cu:635-755 */
static mppi_status computeControlRobust(mppi_handle h, const float* x0_real, int stride)
{
  const int S = h->S;
  if (!h->gains_set)
    return fail(h, MPPI_ERR_STATE, "Robust MPPI: set the DDP feedback gains first (mppi_set_feedback_gains)");
  if (!h->low_latency)
  {
    HIP_TRY(h, hipMemcpyAsync(h->x0_d, h->rm_nominal_state.data(), sizeof(float) * S, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->x0_d + S, x0_real, sizeof(float) * S, hipMemcpyHostToDevice, h->stream));
    // both importance samplers start from the nominal control (:655-656); later iterations continue from the NEW nominal
    HIP_TRY(h, hipMemcpyAsync(h->mean_d, h->nominal_control_h.data(), sizeof(float) * h->TC, hipMemcpyHostToDevice,
                              h->stream));
  }
  if (h->low_latency)
  {
    /* As computeControlVanilla: inputs and results through host memory mapped into the device, no copy command and no stream
     * synchronisation; the call returns when both control sequences and the statistics are out, while the finalize kernel
     * still re-rolls the two state trajectories (the nominal one is what the NEXT call's candidate states are built from:
     * rmNominalStateAndStride and the trajectory getters wait for it).  AutoRally-NN, T = 150: 179 us of a 622 us call. */
    if (h->traj_pending)
      MPPI_TRY(ensureTrajectories(h));
    // both importance samplers start from the nominal control (:655-656), each system smooths with its own history
    const std::vector<float>* const means[2] = { &h->nominal_control_h, &h->nominal_control_h };
    stageInputs(h, h->io_in_h, x0_real, means, h->sys.history, 2 * h->C);
    launchIngest(h);
    HIP_TRY(h, hipGetLastError());
    for (int it = 0; it < h->cfg.num_iters; it++)
    {
      if (it > 0)
        HIP_TRY(h, hipMemcpyAsync(h->mean_d + h->TC, h->mean_d, sizeof(float) * h->TC, hipMemcpyDeviceToDevice, h->stream));
      MPPI_TRY(iteration(h, it, stride));
    }
    // smooth both with their own history, then both state trajectories (:732-737); one launch (no split for this controller)
    kernels::FinalizeArgs a = finalizeArgs(h, h->mean_d, 2 * h->C, /*smooth both*/ 3, 0);
    toOutbox(h, a, 2);
    MPPI_TRY(launchHandover(h, a, 2, nullptr, nullptr));
    MPPI_TRY(takeControls(h, [] {}));
    if (!allFinite(h->control_h) || !allFinite(h->nominal_control_h))
      return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite value in the control sequence");
    return MPPI_OK;
  }
  for (int it = 0; it < h->cfg.num_iters; it++)
  {
    HIP_TRY(h, hipMemcpyAsync(h->mean_d + h->TC, h->mean_d, sizeof(float) * h->TC, hipMemcpyDeviceToDevice, h->stream));
    MPPI_TRY(iteration(h, it, stride));
  }
  // smooth both with their own history, then the nominal state trajectory from the smoothed nominal control (:732-737)
  MPPI_TRY(finalize(h, h->mean_d, /*smooth both*/ 3, /*constrain*/ 0, h->sys.control, h->sys.state));
  MPPI_TRY(fetchStats(h));
  if (!allFinite(h->control_h) || !allFinite(h->nominal_control_h) || !allFinite(h->nominal_state_h))
    return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite value in the control or state sequence");
  return MPPI_OK;
}

mppi_status mppi_compute_control(mppi_handle h, const float* x0, int stride)
{
  CHECK_HANDLE_HOST(h);
  if (!x0 || stride < 0)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_compute_control: null state or negative stride");
  for (int i = 0; i < h->S; i++)  // base_plant.hpp:466-470 skips the iteration on a non-finite state; here the call says so
    if (!std::isfinite(x0[i]))
      return fail(h, MPPI_ERR_NAN, "mppi_compute_control: non-finite initial state");
  RoctxRange range("mppi:compute_control");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  h->last_stride = stride;
  const mppi_status st = h->cfg.controller == MPPI_CONTROLLER_TUBE   ? computeControlTube(h, x0, stride) :
                         h->cfg.controller == MPPI_CONTROLLER_ROBUST ? computeControlRobust(h, x0, stride) :
                                                                       computeControlVanilla(h, x0, stride);
  if (st == MPPI_OK)
    h->have_result = true;
  return st;
}

/* ---------------------------------------------------------------- linearisation ---------------------------------- */
int mppi_has_compute_grad(mppi_handle h)
{
  return h && h->model->hasComputeGrad() ? 1 : 0;
}

/** queues linearizeKernel for the n points x_d[n][S], u_d[n][C] (device memory) behind whatever the stream holds; A and B stay
 *  in h->lin_out_d, where `a` says */
static mppi_status linearizeLaunch(mppi_handle h, const float* x_d, const float* u_d, int n, kernels::LinearizeArgs& a)
{
  const size_t nA = (size_t)n * h->S * h->S, nB = (size_t)n * h->S * h->C;
  if (h->lin_out_d.size() < nA + nB)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // an earlier launch may still write the old buffer
    HIP_TRY(h, h->lin_out_d.alloc(nA + nB));
  }
  a = kernels::LinearizeArgs{};
  a.x_d = x_d;
  a.u_d = u_d;
  a.A_d = h->lin_out_d;
  a.B_d = h->lin_out_d + nA;
  a.n = n;
  std::string err;
  const mppi_status st = h->model->launchLinearize(a, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  return MPPI_OK;
}

/** the Jacobians into the caller's host arrays: one launch, two copies back, one synchronisation */
static mppi_status linearizeOnDevice(mppi_handle h, const float* x_d, const float* u_d, int n, float* A_out, float* B_out)
{
  const size_t nA = (size_t)n * h->S * h->S, nB = (size_t)n * h->S * h->C;
  kernels::LinearizeArgs a{};
  MPPI_TRY(linearizeLaunch(h, x_d, u_d, n, a));
  HIP_TRY(h, hipMemcpyAsync(A_out, a.A_d, sizeof(float) * nA, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(B_out, a.B_d, sizeof(float) * nB, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

/** the caller's points x[n][S], u[n][C] -> h->lin_in_d, queued on the stream */
static mppi_status uploadPoints(mppi_handle h, const float* x, const float* u, int n)
{
  const size_t nx = (size_t)n * h->S, nu = (size_t)n * h->C;
  if (h->lin_in_d.size() < nx + nu)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->lin_in_d.alloc(nx + nu));
  }
  HIP_TRY(h, hipMemcpyAsync(h->lin_in_d, x, sizeof(float) * nx, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->lin_in_d + nx, u, sizeof(float) * nu, hipMemcpyHostToDevice, h->stream));
  return MPPI_OK;
}

mppi_status mppi_linearize(mppi_handle h, const float* x, const float* u, int n, float* A_out, float* B_out)
{
  CHECK_HANDLE(h);
  if (!x || !u || !A_out || !B_out)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_linearize: null pointer");
  if (n <= 0)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_linearize: n must be at least 1");
  if (!h->model->hasComputeGrad())
    return fail(h, MPPI_ERR_UNSUPPORTED, "mppi_linearize: the Dynamics class of model '" + h->model_name + "' declares no computeGrad");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  MPPI_TRY(uploadPoints(h, x, u, n));
  return linearizeOnDevice(h, h->lin_in_d, h->lin_in_d + (size_t)n * h->S, n, A_out, B_out);
}

/** the (state, control) sequence of `system` where the last mppi_compute_control left it on the device, after the refusals
 *  mppi_linearize_trajectory and mppi_compute_feedback share; `who` names the entry point in the message */
static mppi_status trajectoryPoints(mppi_handle h, const char* who, int system, const float*& x_d, const float*& u_d)
{
  if (!h->model->hasComputeGrad())
    return fail(h, MPPI_ERR_UNSUPPORTED,
                std::string(who) + ": the Dynamics class of model '" + h->model_name + "' declares no computeGrad");
  if (system != 0 && !(system == 1 && h->D == 2))
    return fail(h, MPPI_ERR_INVALID_ARG, std::string(who) + ": system 0, or 1 (the nominal system) on a Tube / Robust handle");
  if (!h->have_result)
    return fail(h, MPPI_ERR_STATE, std::string(who) + ": no mppi_compute_control has run on this handle yet");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  // which system of the last finalize pass holds the sequence a getter reports: through the system table, as the getters do
  const std::vector<float>* xs = system == 0 ? h->sys.state[0] : &h->nominal_state_h;
  const std::vector<float>* us = system == 0 ? &h->control_h : &h->nominal_control_h;
  int zx = 0, zu = 0;
  for (int z = 0; z < h->D; z++)
  {
    if (h->sys.state[z] == xs)
      zx = z;
    if (h->sys.control[z] == us)
      zu = z;
  }
  const int T = h->cfg.num_timesteps;
  float* base = h->results_in_io ? h->io_out_h.dev() : h->out_block_d.get();
  x_d = outSlice(base, h->out.state) + (size_t)zx * T * h->S;
  u_d = outSlice(base, h->out.control) + (size_t)zu * h->TC;
  return MPPI_OK;
}

mppi_status mppi_linearize_trajectory(mppi_handle h, int system, float* A_out, float* B_out)
{
  CHECK_HANDLE(h);  // (split hand-over: behind the trajectory phase that writes the state sequence)
  if (!A_out || !B_out)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_linearize_trajectory: null pointer");
  const float *x_d = nullptr, *u_d = nullptr;
  MPPI_TRY(trajectoryPoints(h, "mppi_linearize_trajectory", system, x_d, u_d));
  return linearizeOnDevice(h, x_d, u_d, h->cfg.num_timesteps, A_out, B_out);
}

/* ---------------------------------------------------------------- DDP tracking gains ----------------------------- */
mppi_status mppi_set_feedback_params(mppi_handle h, const float* Q, const float* R, const float* Qf, int num_iterations)
{
  CHECK_HANDLE_HOST(h);
  if (num_iterations != 1)
    return fail(h, MPPI_ERR_UNSUPPORTED,
                "mppi_set_feedback_params: num_iterations = " + std::to_string(num_iterations) +
                    " needs the forward pass and line search of the reference's DDP (ddp/ddp.h:129-162), which are not built; "
                    "only the backward pass of num_iterations = 1 (the DDPParams default) is");
  const int S = h->S, C = h->C;
  std::vector<float>& p = h->fb_params_h;
  p.assign((size_t)2 * S * S + C * C, 0.0f);
  auto fill = [](float* dst, const float* src, int n) {
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++)
        dst[i * n + j] = src ? src[i * n + j] : (i == j ? 1.0f : 0.0f);
  };
  fill(p.data(), Q, S);
  fill(p.data() + S * S, R, C);
  fill(p.data() + S * S + C * C, Qf, S);
  h->fb_params_dirty = true;
  return MPPI_OK;
}

/** linearizeKernel, then ddpBackwardKernel reading its A, B in place, on the handle's stream; the status and (gains_out != null)
 *  the gains come back with one synchronisation.  install: a successful result becomes the model's gains, device to device. */
static mppi_status feedbackOnDevice(mppi_handle h, const char* who, const float* x_d, const float* u_d, bool install,
                                    float* gains_out)
{
  const int T = h->cfg.num_timesteps;
  const size_t nG = (size_t)T * h->S * h->C, nSS = (size_t)h->S * h->S, nCC = (size_t)h->C * h->C;
  if (h->fb_params_h.empty())
    MPPI_TRY(mppi_set_feedback_params(h, nullptr, nullptr, nullptr, 1));  // DDPParams' defaults: identities
  if (h->fb_gains_d.size() < nG || h->fb_params_d.size() < 2 * nSS + nCC || h->fb_status_d.size() < 2)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->fb_gains_d.alloc(nG));
    HIP_TRY(h, h->fb_params_d.alloc(2 * nSS + nCC));
    HIP_TRY(h, h->fb_status_d.alloc(2));
    h->fb_params_dirty = true;
  }
  if (h->fb_params_dirty)
  {
    // pageable source: the copy has left fb_params_h when the call returns
    HIP_TRY(h, hipMemcpyAsync(h->fb_params_d, h->fb_params_h.data(), sizeof(float) * (2 * nSS + nCC), hipMemcpyHostToDevice, h->stream));
    h->fb_params_dirty = false;
  }
  kernels::LinearizeArgs lin{};
  MPPI_TRY(linearizeLaunch(h, x_d, u_d, T, lin));
  kernels::DdpBackwardArgs a{};
  a.A_d = lin.A_d;
  a.B_d = lin.B_d;
  a.Q_d = h->fb_params_d;
  a.R_d = h->fb_params_d + nSS;
  a.Qf_d = h->fb_params_d + nSS + nCC;
  a.gains_d = h->fb_gains_d;
  a.status_d = h->fb_status_d;
  a.dt = h->cfg.dt;
  a.T = T;
  std::string err;
  mppi_status st = h->model->launchDdpBackward(a, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  int status[2] = { 0, 0 };
  if (gains_out)
  {
    h->fb_gains_h.resize(nG);
    HIP_TRY(h, hipMemcpyAsync(h->fb_gains_h.data(), a.gains_d, sizeof(float) * nG, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipMemcpyAsync(status, a.status_d, sizeof(status), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (status[0] != 1)
    return fail(h, MPPI_ERR_NAN,
                std::string(who) + ": the backward pass failed at step " + std::to_string(status[1]) +
                    ": a pivot of quu = R dt + Bd^T Vxx Bd is not positive and finite; no gains were produced or installed");
  if (gains_out)
    std::copy(h->fb_gains_h.begin(), h->fb_gains_h.end(), gains_out);
  if (install)
  {
    st = h->model->setFeedbackGains(h->fb_gains_d, T, h->fb_accumulate_all, true, h->stream, err);
    if (st != MPPI_OK)
      return fail(h, st, err);
    h->gains_set = true;
  }
  return MPPI_OK;
}

mppi_status mppi_compute_feedback(mppi_handle h, int system, float* gains_out)
{
  CHECK_HANDLE(h);  // (split hand-over: behind the trajectory phase that writes the state sequence)
  const bool robust_nominal = h->cfg.controller == MPPI_CONTROLLER_ROBUST && system == 1;
  if (robust_nominal && !h->have_result && h->rm_traj_ready && h->model->hasComputeGrad())
  {
    // a Robust handle cannot run before it has gains: its first ones come from the nominal trajectory
    // mppi_update_importance_sampling_control left on the host (where the reference calls computeNominalFeedbackGains)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int T = h->cfg.num_timesteps;
    MPPI_TRY(uploadPoints(h, h->nominal_state_h.data(), h->nominal_control_h.data(), T));
    return feedbackOnDevice(h, "mppi_compute_feedback", h->lin_in_d, h->lin_in_d + (size_t)T * h->S, true, gains_out);
  }
  const float *x_d = nullptr, *u_d = nullptr;
  MPPI_TRY(trajectoryPoints(h, "mppi_compute_feedback", system, x_d, u_d));
  return feedbackOnDevice(h, "mppi_compute_feedback", x_d, u_d, robust_nominal, gains_out);
}

mppi_status mppi_compute_feedback_at(mppi_handle h, const float* x, const float* u, float* gains_out)
{
  CHECK_HANDLE(h);
  if (!x || !u)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_compute_feedback_at: null pointer");
  if (!h->model->hasComputeGrad())
    return fail(h, MPPI_ERR_UNSUPPORTED,
                "mppi_compute_feedback_at: the Dynamics class of model '" + h->model_name + "' declares no computeGrad");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const int T = h->cfg.num_timesteps;
  MPPI_TRY(uploadPoints(h, x, u, T));
  return feedbackOnDevice(h, "mppi_compute_feedback_at", h->lin_in_d, h->lin_in_d + (size_t)T * h->S, false, gains_out);
}

mppi_status mppi_get_control_seq(mppi_handle h, float* u)
{
  CHECK_HANDLE_HOST(h);
  if (!u)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  std::copy(h->control_h.begin(), h->control_h.end(), u);
  return MPPI_OK;
}
mppi_status mppi_get_state_seq(mppi_handle h, float* x)
{
  CHECK_HANDLE_HOST(h);
  if (!x)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  MPPI_TRY(ensureTrajectories(h));
  // system 0: RobustMPPI::getTargetStateSeq returns the nominal state trajectory (robust_mppi_controller.cuh:131-134)
  const std::vector<float>& src = *h->sys.state[0];
  std::copy(src.begin(), src.end(), x);
  return MPPI_OK;
}
mppi_status mppi_get_output_seq(mppi_handle h, float* y)
{
  CHECK_HANDLE_HOST(h);
  if (!y)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_get_output_seq: null");
  // system 0 of the last finalize pass is the trajectory mppi_get_state_seq reports (real system for Vanilla / Tube, the
  // nominal one for Robust MPPI)
  if (h->results_in_io)
  {  // the last finalize pass wrote its outputs to the device-mapped host block
    MPPI_TRY(ensureTrajectories(h));
    const float* src = outSlice(h->io_out_h, h->out.output);
    std::copy(src, src + (size_t)h->cfg.num_timesteps * h->O, y);
    return MPPI_OK;
  }
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  joinSideStream(h);
  HIP_TRY(h, hipMemcpyAsync(y, h->output_out_d, sizeof(float) * h->cfg.num_timesteps * h->O, hipMemcpyDeviceToHost,
                            h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

mppi_status mppi_get_nominal_control_seq(mppi_handle h, float* u)
{
  CHECK_HANDLE_HOST(h);
  if (!u)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  if (h->D != 2)
    return fail(h, MPPI_ERR_STATE, "no nominal system in this controller");
  std::copy(h->nominal_control_h.begin(), h->nominal_control_h.end(), u);
  return MPPI_OK;
}
mppi_status mppi_get_nominal_state_seq(mppi_handle h, float* x)
{
  CHECK_HANDLE_HOST(h);
  if (!x)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  if (h->D != 2)
    return fail(h, MPPI_ERR_STATE, "no nominal system in this controller");
  MPPI_TRY(ensureTrajectories(h));
  std::copy(h->nominal_state_h.begin(), h->nominal_state_h.end(), x);
  return MPPI_OK;
}

/** reference: controllers/controller.cuh:602-615 */
static void saveControlHistory(int steps, const std::vector<float>& u, std::vector<float>& hist, int C)
{
  if (steps == 1)
  {
    for (int c = 0; c < C; c++)
    {
      hist[c] = hist[C + c];
      hist[C + c] = u[c];
    }
  }
  else if (steps >= 2)
  {
    for (int c = 0; c < C; c++)
    {
      hist[c] = u[(size_t)(steps - 2) * C + c];
      hist[C + c] = u[(size_t)(steps - 1) * C + c];
    }
  }
}
/** reference: controllers/controller.cuh:588-600 */
static void slideSequence(std::vector<float>& u, int T, int C, int steps, const float* zero, const float* scale)
{
  for (int i = 0; i < T; i++)
  {
    const int ind = std::min(i + steps, T - 1);
    for (int c = 0; c < C; c++)
    {
      u[(size_t)i * C + c] = u[(size_t)ind * C + c];
      if (i + steps > T - 1)
        u[(size_t)i * C + c] = (u[(size_t)ind * C + c] - zero[c]) * scale[c] + zero[c];
    }
  }
}

/** x <- one model step under u (u <- the clamped control when `enforce`), in host memory mapped into the device: no copy
 *  command; the host spins on a flag raised behind the kernel (MPPI_AMD_NO_SPIN=1: a stream synchronisation instead) */
mppi_status modelStepInPlace(mppi_handle h, float* x, float* u, float dt, int enforce)
{
  std::copy(x, x + h->S, h->step_pin_h.get());
  std::copy(u, u + h->C, h->step_pin_h + h->S);
  std::string err;
  mppi_status st = h->model->launchModelStep(h->step_pin_h.dev(), h->step_pin_h.dev() + h->S, dt, enforce, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  MPPI_TRY(streamRoundTrip(h, 8, h->step_seq));
  std::copy(h->step_pin_h.get(), h->step_pin_h + h->S, x);
  std::copy(h->step_pin_h + h->S, h->step_pin_h + h->S + h->C, u);
  return MPPI_OK;
}

mppi_status mppi_slide(mppi_handle h, int steps)
{
  CHECK_HANDLE_HOST(h);
  const int T = h->cfg.num_timesteps, C = h->C;
  if (steps < 0 || steps > T)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_slide: steps out of range");
  if (h->cfg.controller == MPPI_CONTROLLER_ROBUST)
    return MPPI_OK;  // slideControlSequence is empty there (robust_mppi_controller.cuh:178): the slide is part of
                     // updateImportanceSamplingControl
  std::vector<float> zero(C);
  h->model->getZeroControl(zero.data());
  if (h->cfg.controller == MPPI_CONTROLLER_TUBE)
  {
    // tube_mppi_controller.cu:312-323: updateNominalState(nominal_control.col(0)) — one in-place model step, no clamp
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // single launch: the step queues behind the last finalize kernel anyway, and a later trajectory read must not find io_out
    // rewritten — take the trajectories now.  Split hand-over: the step runs beside the trajectory phase
    if (!h->split_finalize)
      MPPI_TRY(ensureTrajectories(h));
    std::vector<float> u0(h->nominal_control_h.begin(), h->nominal_control_h.begin() + C);
    MPPI_TRY(modelStepInPlace(h, h->tube_x_h.data(), u0.data(), h->cfg.dt, 0));
    saveControlHistory(steps, h->nominal_control_h, h->history_h, C);
    slideSequence(h->nominal_control_h, T, C, steps, zero.data(), h->slide_scale_h.data());
    slideSequence(h->control_h, T, C, steps, zero.data(), h->slide_scale_h.data());
    return MPPI_OK;
  }
  saveControlHistory(steps, h->control_h, h->history_h, C);
  slideSequence(h->control_h, T, C, steps, zero.data(), h->slide_scale_h.data());
  return MPPI_OK;
}


/* ---------------------------------------------------------------- Robust MPPI API -------------------------------- */
mppi_status mppi_set_rmppi_params(mppi_handle h, float value_function_threshold, int num_candidates,
                                  int samples_per_candidate)
{
  CHECK_HANDLE(h);
  if (h->cfg.controller != MPPI_CONTROLLER_ROBUST)
    return fail(h, MPPI_ERR_STATE, "mppi_set_rmppi_params: the handle is not a Robust MPPI controller");
  // updateNumCandidates (robust_mppi_controller.cu:414-448): odd, >= 3, candidates * samples <= NUM_ROLLOUTS
  if (num_candidates < 3)
    return fail(h, MPPI_ERR_INVALID_ARG, "ERROR: number of candidates must be greater or equal to 3");
  if (num_candidates % 2 == 0)
    return fail(h, MPPI_ERR_INVALID_ARG, "ERROR: number of candidates must be odd");
  if (samples_per_candidate <= 0 || (long long)num_candidates * samples_per_candidate > h->cfg.num_rollouts)
    return fail(h, MPPI_ERR_INVALID_ARG, "ERROR: (number of candidates) * (SAMPLES_PER_CANDIDATE) cannot exceed NUM_ROLLOUTS");
  h->value_function_threshold = value_function_threshold;
  h->num_candidates = num_candidates;
  h->samples_per_candidate = samples_per_candidate;
  return MPPI_OK;
}

mppi_status mppi_set_feedback_gains(mppi_handle h, const float* gains, int accumulate_all_states)
{
  CHECK_HANDLE(h);
  if (!gains)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_set_feedback_gains: null");
  if (h->cfg.controller != MPPI_CONTROLLER_ROBUST)
    return fail(h, MPPI_ERR_STATE, "mppi_set_feedback_gains: the handle is not a Robust MPPI controller");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  std::string err;
  mppi_status st = h->model->setFeedbackGains(gains, h->cfg.num_timesteps, accumulate_all_states != 0, false, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  h->gains_set = true;
  h->fb_accumulate_all = accumulate_all_states != 0;
  return MPPI_OK;
}

/** reference: robust_mppi_controller.cu:548-568 (updateImportanceSamplingControl); the DDP gain computation at its end
 *  (computeNominalFeedbackGains) is the caller's: mppi_set_feedback_gains */
mppi_status mppi_update_importance_sampling_control(mppi_handle h, const float* state, int stride)
{
  CHECK_HANDLE(h);
  if (!state || stride < 0)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_update_importance_sampling_control: null state or negative stride");
  if (h->cfg.controller != MPPI_CONTROLLER_ROBUST)
    return fail(h, MPPI_ERR_STATE, "mppi_update_importance_sampling_control: the handle is not a Robust MPPI controller");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  MPPI_TRY(ensureTrajectories(h));  // the nominal state trajectory of the last mppi_compute_control (low-latency hand-over)
  const int T = h->cfg.num_timesteps, C = h->C;
  h->real_stride = stride;
  MPPI_TRY(rmNominalStateAndStride(h, state, stride));
  saveControlHistory(h->nominal_stride, h->nominal_control_h, h->nominal_history_h, C);
  saveControlHistory(h->real_stride, h->control_h, h->history_h, C);
  std::vector<float> zero(C);
  h->model->getZeroControl(zero.data());
  slideSequence(h->nominal_control_h, T, C, h->nominal_stride, zero.data(), h->slide_scale_h.data());
  MPPI_TRY(rmNominalStateTrajectory(h));
  h->rm_traj_ready = true;
  return MPPI_OK;
}

mppi_status mppi_get_rmppi_state(mppi_handle h, float* nominal_state, int* best_index, int* nominal_stride,
                                 float* candidate_free_energy)
{
  CHECK_HANDLE(h);
  if (h->cfg.controller != MPPI_CONTROLLER_ROBUST)
    return fail(h, MPPI_ERR_STATE, "mppi_get_rmppi_state: the handle is not a Robust MPPI controller");
  if (nominal_state)
    std::copy(h->rm_nominal_state.begin(), h->rm_nominal_state.end(), nominal_state);
  if (best_index)
    *best_index = h->best_index;
  if (nominal_stride)
    *nominal_stride = h->nominal_stride;
  if (candidate_free_energy)
    for (int i = 0; i < h->num_candidates; i++)
      candidate_free_energy[i] = i < (int)h->rm_cand_free_energy.size() ? h->rm_cand_free_energy[i] : 0.0f;
  return MPPI_OK;
}

mppi_status mppi_get_costs(mppi_handle h, float* costs)
{
  CHECK_HANDLE(h);
  if (!costs)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  HIP_TRY(h, hipMemcpyAsync(costs, h->costs_d, sizeof(float) * h->D * h->K_local, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}
mppi_status mppi_get_stats(mppi_handle h, mppi_stats* out)
{
  CHECK_HANDLE_HOST(h);
  if (!out)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  if (!h->stats_h_fresh)
  {  // a read from the device: behind everything, the side stream included
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    joinSideStream(h);
  }
  const int used = h->stats_h.nominal_state_used;
  MPPI_TRY(fetchStats(h));
  h->stats_h.nominal_state_used = used;
  *out = h->stats_h;
  if (h->exchange_failed)
    return fail(h, MPPI_ERR_COMM, "P2P exchange: a peer's record did not arrive within 2 s; the merge was abandoned");
  return MPPI_OK;
}
mppi_status mppi_get_sampled_controls(mppi_handle h, float* v)
{
  CHECK_HANDLE(h);
  if (!v)
    return fail(h, MPPI_ERR_INVALID_ARG, "null");
  if (!h->samples_d)
    return fail(h, MPPI_ERR_STATE, "mppi_get_sampled_controls: handle was created without save_samples");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  HIP_TRY(h, hipMemcpyAsync(v, h->samples_d, sizeof(float) * h->D * h->K_local * h->TC, hipMemcpyDeviceToHost,
                            h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

mppi_status mppi_sample_noise(mppi_handle h, int optimization_stride, float* eps_out)
{
  CHECK_HANDLE(h);
  if (!eps_out || optimization_stride < 0)
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_sample_noise: bad arguments");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  SamplerLaunchState s{};
  s.num_rollouts_local = h->K_local;
  s.num_rollouts_global = h->cfg.num_rollouts;
  s.rollout_offset = h->K_offset;
  s.num_timesteps = h->cfg.num_timesteps;
  s.num_distributions = 1;
  s.control_means_d = h->mean_d;
  s.eps_d = nullptr;
  if (h->noise_source == MPPI_NOISE_INJECTED)
  {
    if (!h->eps_d || h->n_eps_iters <= 0)
      return fail(h, MPPI_ERR_STATE, "noise source is MPPI_NOISE_INJECTED but no noise has been injected");
    s.eps_d = h->eps_d + (size_t)(h->generation % (uint32_t)h->n_eps_iters) * epsFloatsPerIteration(h);
  }
  else if (h->noise_source == MPPI_NOISE_ROCRAND_HOST)
    return fail(h, MPPI_ERR_UNSUPPORTED, "this call draws through the sampler's random-access path: use the Philox or the "
                                         "injected noise source (MPPI_NOISE_ROCRAND_HOST fills the rollout kernel's eps buffer only)");
  s.control_samples_d = nullptr;
  s.seed = h->cfg.seed;
  s.generation = h->generation;
  s.iteration = 0;
  s.optimization_stride = optimization_stride;
  s.independent_noise = h->independent_noise ? 1 : 0;
  const size_t n = (size_t)h->K_local * h->TC;
  HipBuffer<float> out_d;
  HIP_TRY(h, out_d.alloc(n));
  std::string err;
  mppi_status st = h->model->launchNoiseDump(s, out_d, h->stream, err);
  hipError_t e = hipSuccess;
  if (st == MPPI_OK)
  {
    e = hipMemcpyAsync(eps_out, out_d, n * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
      e = hipStreamSynchronize(h->stream);
  }
  if (st != MPPI_OK)
    return fail(h, st, err);
  if (e != hipSuccess)
    return fail(h, MPPI_ERR_HIP, std::string("mppi_sample_noise: ") + hipGetErrorString(e));
  return MPPI_OK;
}
