/**
 * engine_replay.hip — what the sampled rollouts of the last iteration did: the n best of them selected on the device
 * (mppi_top_rollouts, engine/top_rollouts_kernel.hpp) and chosen rows run again with their outputs, step costs and crash flags
 * kept (mppi_replay_rollouts, engine/replay_kernel.hpp).  Off the mppi_compute_control / mppi_optimize path: both queue behind
 * whatever is on the handle's stream, and nothing the controller computes depends on them.
 * Part of the implementation of include/mppi_amd.h; see engine_internal.hpp for how the engine is divided.
 */
#include "engine_internal.hpp"
#include "mppi_amd/engine/top_rollouts_kernel.hpp"
#include "mppi_amd/engine/replay_host.hpp"

static_assert(mppi::replay::TOP_N_MAX == mppi::kernels::TOP_ROLLOUTS_MAX, "the host check and the kernel's LDS array agree");

/** the rule of mppi_linearize_trajectory */
static bool systemExists(const mppi_handle_s* h, int system)
{
  return system == 0 || (system == 1 && h->D == 2);
}

mppi_status mppi_top_rollouts(mppi_handle h, int system, int n, int* idx_out, float* cost_out)
{
  CHECK_HANDLE(h);
  if (!systemExists(h, system))
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_top_rollouts: system 0, or 1 (the nominal system) on a Tube / Robust handle");
  const std::string refusal = mppi::replay::checkTopN(n, h->K_local);
  if (!refusal.empty())
    return fail(h, MPPI_ERR_INVALID_ARG, refusal);
  if (h->n_rollout_launches == 0)
    return fail(h, MPPI_ERR_STATE, "mppi_top_rollouts: no iteration has run on this handle yet");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (h->top_d.size() < 2 * (size_t)n)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->top_d.alloc(2 * (size_t)mppi::replay::TOP_N_MAX));
  }
  int* idx_d = reinterpret_cast<int*>(h->top_d.get());
  float* cost_d = h->top_d.get() + n;
  hipLaunchKernelGGL(kernels::topRolloutsKernel, dim3(1), dim3(kernels::TOP_ROLLOUTS_THREADS), 0, h->stream,
                     h->costs_d.get() + (size_t)system * h->K_local, h->K_local, n, idx_d, cost_d);
  HIP_TRY(h, hipGetLastError());
  h->replay_h.resize(2 * (size_t)n);
  HIP_TRY(h, hipMemcpyAsync(h->replay_h.data(), h->top_d, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (idx_out)
    memcpy(idx_out, h->replay_h.data(), sizeof(int) * n);
  if (cost_out)
    memcpy(cost_out, h->replay_h.data() + n, sizeof(float) * n);
  return MPPI_OK;
}

mppi_status mppi_replay_rollouts(mppi_handle h, int system, const int* rollout_idx, int n, float* y_out, float* step_cost_out,
                                 int* crash_out)
{
  CHECK_HANDLE(h);  // (split hand-over: behind the trajectory phase and the copy of the call's inputs)
  if (h->cfg.controller == MPPI_CONTROLLER_ROBUST)
    return fail(h, MPPI_ERR_UNSUPPORTED, "mppi_replay_rollouts: the real system's rollouts of a Robust MPPI handle carry the "
                                         "feedback term, which is not replayed");
  if (!systemExists(h, system))
    return fail(h, MPPI_ERR_INVALID_ARG, "mppi_replay_rollouts: system 0, or 1 (the nominal system) on a Tube handle");
  bool needs_samples = false, needs_optimal = false;
  const std::string refusal = mppi::replay::checkReplayIndices(rollout_idx, n, h->K_local, needs_samples, needs_optimal);
  if (!refusal.empty())
    return fail(h, MPPI_ERR_INVALID_ARG, refusal);
  if (h->n_rollout_launches == 0)
    return fail(h, MPPI_ERR_STATE, "mppi_replay_rollouts: no iteration has run on this handle yet");
  if (needs_samples && !h->samples_d)
    return fail(h, MPPI_ERR_STATE, "mppi_replay_rollouts: handle was created without save_samples");
  if (needs_optimal && !h->have_result)
    return fail(h, MPPI_ERR_STATE, "mppi_replay_rollouts: index -1 is the control sequence of a mppi_compute_control, and none "
                                   "has run on this handle yet");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  MPPI_TRY(flushMerge(h));  // the mean the likelihood-ratio term reads (streamed merge: the last records may be un-merged)

  const int T = h->cfg.num_timesteps, O = h->O;
  // one device block: results [y | step costs | crash flags], then the index list
  const size_t ny = (size_t)n * T * O, nc = (size_t)n * (T + 1), nf = (size_t)n * T;
  const size_t words = ny + nc + nf + (size_t)n;
  if (h->replay_d.size() < words)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->replay_d.alloc(words));
  }
  float* base = h->replay_d.get();
  int* idx_d = reinterpret_cast<int*>(base + ny + nc + nf);
  HIP_TRY(h, hipMemcpyAsync(idx_d, rollout_idx, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));

  kernels::ReplayArgs a{};
  a.x0_d = h->x0_d + (size_t)system * h->S;
  a.samples_d = h->samples_d ? h->samples_d.get() + (size_t)system * h->K_local * h->TC : nullptr;
  {
    // the control sequence a getter reports for this system, where the last finalize pass left it (mppi_linearize_trajectory)
    const std::vector<float>* us = system == 0 ? &h->control_h : &h->nominal_control_h;
    int zu = 0;
    for (int z = 0; z < h->D; z++)
      if (h->sys.control[z] == us)
        zu = z;
    float* out_base = h->results_in_io ? h->io_out_h.dev() : h->out_block_d.get();
    a.optimal_d = outSlice(out_base, h->out.control) + (size_t)zu * h->TC;
  }
  a.idx_d = idx_d;
  a.y_d = base;
  a.cost_d = base + ny;
  a.crash_d = reinterpret_cast<int*>(base + ny + nc);
  a.n = n;
  a.num_timesteps = T;
  a.system = system;
  a.dt = h->cfg.dt;
  a.lambda = h->cfg.lambda;
  a.alpha = h->cfg.alpha;

  SamplerLaunchState s{};
  s.num_rollouts_local = h->K_local;
  s.num_rollouts_global = h->cfg.num_rollouts;
  s.rollout_offset = h->K_offset;
  s.num_timesteps = T;
  s.num_distributions = h->D;
  s.control_means_d = h->mean_d;
  s.eps_d = nullptr;
  s.control_samples_d = nullptr;
  s.seed = h->cfg.seed;
  s.generation = h->generation;
  s.iteration = 0;
  s.optimization_stride = h->last_stride;
  s.independent_noise = h->independent_noise ? 1 : 0;
  std::string err;
  const mppi_status st = h->model->launchReplay(a, s, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  h->replay_h.resize(ny + nc + nf);
  HIP_TRY(h, hipMemcpyAsync(h->replay_h.data(), base, sizeof(float) * (ny + nc + nf), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (y_out)
    memcpy(y_out, h->replay_h.data(), sizeof(float) * ny);
  if (step_cost_out)
    memcpy(step_cost_out, h->replay_h.data() + ny, sizeof(float) * nc);
  if (crash_out)
    memcpy(crash_out, h->replay_h.data() + ny + nc, sizeof(int) * nf);
  return MPPI_OK;
}
