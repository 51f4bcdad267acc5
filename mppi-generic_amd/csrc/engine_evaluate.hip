/**
 * engine_evaluate.hip — control sequences the caller brings: what they would cost (mppi_evaluate_controls) and whether one of
 * them should replace the handle's current sequence (mppi_warm_start), both one launch of engine/evaluate_kernel.hpp.  Off the
 * mppi_compute_control / mppi_optimize path: they queue behind whatever is on the handle's stream, and nothing the controller
 * computes depends on mppi_evaluate_controls; mppi_warm_start changes the handle the way mppi_set_nominal_control does, or not at all.
 * Part of the implementation of include/mppi_amd.h; see engine_internal.hpp for how the engine is divided.
 */
#include "engine_internal.hpp"
#include "mppi_amd/engine/evaluate_host.hpp"

/** rows[0 .. n_head) <- head (one row, may be null with n_head == 0), the next n_tail rows <- tail, the states <- x0[x0_count][S]:
 *  one launch, then costs and crash flags in h->eval_h as [n] floats | [n] ints, n = n_head + n_tail */
static mppi_status evaluateRows(mppi_handle h, const float* x0, int x0_count, const float* head, int n_head, const float* tail,
                                int n_tail)
{
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const int n = n_head + n_tail;
  const size_t nu = (size_t)n * h->TC, nx = (size_t)x0_count * h->S;
  const size_t words = nu + nx + 2 * (size_t)n;
  if (h->eval_d.size() < words)
  {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->eval_d.alloc(words));
  }
  float* base = h->eval_d.get();
  if (n_head)
    HIP_TRY(h, hipMemcpyAsync(base, head, sizeof(float) * n_head * h->TC, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(base + (size_t)n_head * h->TC, tail, sizeof(float) * n_tail * h->TC, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(base + nu, x0, sizeof(float) * nx, hipMemcpyHostToDevice, h->stream));

  kernels::EvaluateArgs a{};
  a.x0_d = base + nu;
  a.x0_stride = x0_count == 1 ? 0 : h->S;
  a.u_d = base;
  a.cost_d = base + nu + nx;
  a.crash_d = reinterpret_cast<int*>(base + nu + nx + n);
  a.n = n;
  a.num_timesteps = h->cfg.num_timesteps;
  a.dt = h->cfg.dt;
  std::string err;
  const mppi_status st = h->model->launchEvaluate(a, h->stream, err);
  if (st != MPPI_OK)
    return fail(h, st, err);
  h->eval_h.resize(2 * (size_t)n);
  HIP_TRY(h, hipMemcpyAsync(h->eval_h.data(), a.cost_d, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

mppi_status mppi_evaluate_controls(mppi_handle h, const float* x0, int x0_count, const float* u, int n, float* cost_out,
                                   int* crash_out)
{
  // the arguments first: a refusal that needs no handle reads the same with or without one (mppi_last_error(NULL) then has it)
  const std::string refusal = mppi::evaluate::checkEvaluateArgs(x0, x0_count, u, n);
  if (!h)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, refusal.empty() ? "mppi_evaluate_controls: null handle" : refusal);
  CHECK_HANDLE(h);
  if (!refusal.empty())
    return fail(h, MPPI_ERR_INVALID_ARG, refusal);
  MPPI_TRY(evaluateRows(h, x0, x0_count, nullptr, 0, u, n));
  if (cost_out)
    memcpy(cost_out, h->eval_h.data(), sizeof(float) * n);
  if (crash_out)
    memcpy(crash_out, h->eval_h.data() + n, sizeof(int) * n);
  return MPPI_OK;
}

mppi_status mppi_warm_start(mppi_handle h, const float* x0, const float* candidates, int n, float hysteresis, int* chosen_out,
                            float* cost_out)
{
  const std::string refusal = mppi::evaluate::checkWarmStartArgs(x0, candidates, n, hysteresis);
  if (!h)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, refusal.empty() ? "mppi_warm_start: null handle" : refusal);
  CHECK_HANDLE(h);
  if (h->cfg.controller == MPPI_CONTROLLER_ROBUST)
    return fail(h, MPPI_ERR_UNSUPPORTED, mppi::evaluate::warmStartRobustRefusal());
  if (!refusal.empty())
    return fail(h, MPPI_ERR_INVALID_ARG, refusal);
  // row 0: the sequence mppi_get_control_seq returns now (the host's copy, after any mppi_slide)
  MPPI_TRY(evaluateRows(h, x0, 1, h->control_h.data(), 1, candidates, n));
  const float* costs = h->eval_h.data();
  const int chosen = mppi::evaluate::warmStartChoice(costs, n, hysteresis);
  if (chosen >= 0)
    MPPI_TRY(mppi_set_nominal_control(h, candidates + (size_t)chosen * h->TC));
  if (chosen_out)
    *chosen_out = chosen;
  if (cost_out)
    memcpy(cost_out, costs, sizeof(float) * ((size_t)n + 1));
  return MPPI_OK;
}
