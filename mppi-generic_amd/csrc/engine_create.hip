/**
 * engine_create.hip — mppi_create / mppi_create_with_sampler: the checks in their order, the launch plan (launch_plan.hpp), and
 * the handle's buffers.  Every failure returns: the unique_ptr deletes the handle, ~mppi_handle_s (engine_core.hip) and the
 * owning members release what exists.
 */
#include "engine_internal.hpp"
#include "launch_plan.hpp"

static bool envIs(const char* name, char value)
{
  const char* v = getenv(name);
  return v && v[0] == value;
}
static bool envFlag(const char* name)
{
  return envIs(name, '1');
}

/** the environment switches mppi_create reads (engine_internal.hpp says what each does, at the handle field it sets) */
struct CreateSwitches
{
  bool rows_in_hbm = envFlag("MPPI_AMD_ROWS_IN_HBM");            // test hook: the HBM-row variant at any horizon
  bool no_spin = envFlag("MPPI_AMD_NO_SPIN");
  bool no_bar_inbox = envIs("MPPI_AMD_BAR_INBOX", '0');
  bool no_stream_merge = envFlag("MPPI_AMD_NO_STREAM_MERGE");
  bool no_merge_control = envFlag("MPPI_AMD_NO_MERGE_CONTROL");
  bool finalize_scratch = envFlag("MPPI_AMD_FINALIZE_SCRATCH");  // test hook: the finalize kernels' sequences in HBM
  bool no_split_finalize = envIs("MPPI_AMD_SPLIT_FINALIZE", '0');
  const char* reduction = getenv("MPPI_AMD_REDUCTION");
};

static mppi_status checkArguments(const mppi_config* cfg, int sampler_kind, mppi_handle* out)
{
  if (!cfg || !out || !cfg->model)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: null argument");
  *out = nullptr;
  {  // which sampler a controller kind takes: the plan's rule (launch_plan.hpp), asked here so that a mismatch is reported
     // before the sizes and before a device is looked for; an unknown controller kind is reported by the plan
    std::string refusal;
    const mppi_status rule = plan::samplerRule(cfg->controller, sampler_kind, &refusal);
    if (rule != MPPI_OK)
      return fail(nullptr, rule, refusal);
  }
  if (cfg->num_rollouts <= 0 || cfg->num_timesteps <= 0 || !(cfg->dt > 0.0f) || !(cfg->lambda > 0.0f) ||
      cfg->num_iters <= 0)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: num_rollouts, num_timesteps, dt, lambda, num_iters must be > 0");
  if (cfg->kernel_variant < 0 || cfg->kernel_variant > MPPI_KERNEL_PIPELINE)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: unknown kernel_variant");
  const int world = cfg->world_size > 0 ? cfg->world_size : 1;
  if (cfg->rank < 0 || cfg->rank >= world || cfg->num_rollouts % world != 0)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: rank/world_size invalid or num_rollouts not divisible by world_size");
  return MPPI_OK;
}

static mppi_status checkDevice(const mppi_config& cfg)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, MPPI_ERR_NO_DEVICE, "mppi_create: no HIP device visible (this library has no CPU path)");
  if (cfg.device < 0 || cfg.device >= ndev)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: device ordinal out of range");
  return MPPI_OK;
}

/** the model instantiation for (name, sampler kind), or which of the three ways it is missing; then what the instantiation
 *  itself rules out */
static mppi_status resolveModel(const mppi_config& cfg, const std::string& name, int sampler_kind, std::unique_ptr<ModelBase>& model)
{
  // Tube with the colored sampler: the model's two-system registration; without one, its colored registration (the templated
  // controllers list their two-system shapes there) — the plan then says whether that has a shape for two systems
  const int key = plan::registrationKind(cfg.controller, sampler_kind);
  if (key != sampler_kind)
    model.reset(makeModel(name, key));
  if (!model)
    model.reset(makeModel(name, sampler_kind));
  const auto gaussianExists = [&] { return std::unique_ptr<ModelBase>(makeModel(name, MPPI_SAMPLER_GAUSSIAN)) != nullptr; };
  if (!model && sampler_kind == MPPI_SAMPLER_COLORED && gaussianExists())
    return fail(nullptr, MPPI_ERR_UNSUPPORTED, "mppi_create: model '" + name + "' has no colored-noise instantiation");
  if (!model && sampler_kind == MPPI_SAMPLER_NLN && gaussianExists())
    return fail(nullptr, MPPI_ERR_UNKNOWN_MODEL, "mppi_create: model '" + name + "' has no NLN-sampler instantiation "
                                                 "(register one with MPPI_SAMPLER_NLN)");
  if (!model)
    return fail(nullptr, MPPI_ERR_UNKNOWN_MODEL, "mppi_create: model '" + name + "' is not registered; have:\n" + mppi_list_models());
  if (sampler_kind == MPPI_SAMPLER_NLN && cfg.noise_source == MPPI_NOISE_ROCRAND_HOST)
    return fail(nullptr, MPPI_ERR_UNSUPPORTED,
                "mppi_create: MPPI_NOISE_ROCRAND_HOST with the NLN sampler: the host generator fills one normal tensor, the NLN "
                "noise is the product of a normal and a log-normal draw — use MPPI_NOISE_PHILOX_FUSED or inject eps' itself");
  // whichever way the model got into the table: role-separated kernels only for plugins that declare barrier-free steps
  const std::string undeclared = model->undeclaredBarrierFreePlugins();
  if (!undeclared.empty())
    return fail(nullptr, MPPI_ERR_INVALID_ARG,
                "mppi_create: model '" + name + "' carries role-separated rollout kernels but these plugin classes do "
                "not declare MPPI_BARRIER_FREE_STEP (mppi_amd/plugin/parallel_utils.hpp): " + undeclared +
                "— a block barrier inside a per-step method would hang the GPU there; declare it or register with PIPELINE = false");
  return MPPI_OK;
}

static mppi_status allocZeroed(mppi_handle h, HipBuffer<float>& b, size_t n, const char* name)
{
  hipError_t e = b.alloc(n);
  if (e == hipSuccess)
    e = hipMemsetAsync(b, 0, n * sizeof(float), h->stream);
  return e == hipSuccess ? MPPI_OK : fail(nullptr, MPPI_ERR_HIP, std::string("hipMalloc ") + name + ": " + hipGetErrorString(e));
}

/** the input block (x0 | mean | history) and the output block (control | state | output | stats) on the device, their pinned
 *  and device-mapped mirrors, and the inbox in device memory behind the PCIe BAR where the device offers it */
static mppi_status allocHandOver(mppi_handle h, const CreateSwitches& sw)
{
  const int T = h->cfg.num_timesteps, D = h->D, S = h->S, C = h->C;
  auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  h->in.mean.floats = pad4((size_t)D * S);
  h->in.history.floats = h->in.mean.floats + pad4((size_t)D * T * C);
  h->in_floats = h->in.history.floats + pad4((size_t)4 * C);  // history: [2 systems][2][C] (RMPPI smooths both with their own)
  MPPI_TRY(allocZeroed(h, h->in_block_d, h->in_floats, "in_block_d"));
  h->x0_d = inSlice(h->in_block_d, h->in.x0);
  h->mean_d = inSlice(h->in_block_d, h->in.mean);
  h->history_d = inSlice(h->in_block_d, h->in.history);
  h->out.state.floats = pad4((size_t)D * T * C);
  h->out.output.floats = h->out.state.floats + pad4((size_t)D * T * S);
  h->out.stats.floats = h->out.output.floats + pad4((size_t)D * T * h->O);
  h->out_floats = h->out.stats.floats + pad4((size_t)D * kernels::STATS_STRIDE);
  MPPI_TRY(allocZeroed(h, h->out_block_d, h->out_floats, "out_block_d"));
  h->ctrl_out_d = outSlice(h->out_block_d, h->out.control);
  h->state_out_d = outSlice(h->out_block_d, h->out.state);
  h->output_out_d = outSlice(h->out_block_d, h->out.output);
  h->stats_d = outSlice(h->out_block_d, h->out.stats);
  if (h->in_pin_h.allocHost(h->in_floats, hipHostMallocDefault) != hipSuccess ||
      h->out_pin_h.allocHost(h->out_floats, hipHostMallocDefault) != hipSuccess)
    return fail(nullptr, MPPI_ERR_HIP, "hipHostMalloc of the pinned hand-over buffers failed");
  memset(h->in_pin_h, 0, h->in_floats * sizeof(float));
  memset(h->out_pin_h, 0, h->out_floats * sizeof(float));
  h->low_latency = !sw.no_spin;
  const unsigned map_flags = hipHostMallocMapped | hipHostMallocCoherent;
  int large_bar = 0;
  if (h->low_latency && !sw.no_bar_inbox &&
      hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, h->cfg.device) == hipSuccess && large_bar &&
      h->io_in_h.allocExt(h->in_floats, hipDeviceMallocFinegrained) == hipSuccess)
    h->bar_inbox = true;
  else
    (void)hipGetLastError();
  if ((!h->bar_inbox && h->io_in_h.allocHost(h->in_floats, map_flags) != hipSuccess) ||
      h->io_out_h.allocHost(h->out_floats, map_flags) != hipSuccess ||
      h->io_flags_h.allocHost(64 / sizeof(unsigned), map_flags) != hipSuccess)
    return fail(nullptr, MPPI_ERR_HIP, "hipHostMalloc of the device-mapped hand-over buffers failed");
  memset(h->io_in_h, 0, h->in_floats * sizeof(float));
  memset(h->io_out_h, 0, h->out_floats * sizeof(float));
  memset(h->io_flags_h, 0, 64);
  return MPPI_OK;
}

/** costs, block records, exchange buffers, the model-step pair, and on request the samples and the sampler's rows in HBM */
static mppi_status allocWorkBuffers(mppi_handle h)
{
  const int T = h->cfg.num_timesteps, D = h->D, S = h->S, C = h->C, K = h->K_local, world = h->cfg.world_size;
  MPPI_TRY(allocZeroed(h, h->costs_d, (size_t)D * K, "costs_d"));
  // (+ the transposed copy of a one-system launch's records behind them: recordsTransposed(), RolloutArgs::records_t_d)
  const size_t records = (size_t)D * h->num_blocks * h->PS + kernels::transposedRecordFloats(T, C, h->num_blocks);
  MPPI_TRY(allocZeroed(h, h->partials_d, records, "partials_d"));
  MPPI_TRY(allocZeroed(h, h->partials_alt_d, records, "partials_alt_d"));
  MPPI_TRY(allocZeroed(h, h->send_d, (size_t)D * h->PS, "send_d"));
  MPPI_TRY(allocZeroed(h, h->recv_d, (size_t)world * D * h->PS, "recv_d"));
  MPPI_TRY(allocZeroed(h, h->gather_tmp_d, (size_t)world * D * h->PS, "gather_tmp_d"));
  MPPI_TRY(allocZeroed(h, h->ctrl_in_d, (size_t)D * T * C, "ctrl_in_d"));
  MPPI_TRY(allocZeroed(h, h->step_x_d, (size_t)S + C, "step_x_d"));  // [x | u] of mppi_model_step
  h->step_u_d = h->step_x_d + S;
  // [x | u] of a single model step, mapped into the device: the kernel reads and writes it in place, the host waits on a flag
  if (h->step_pin_h.allocHost((size_t)S + C, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return fail(nullptr, MPPI_ERR_HIP, "hipHostMalloc of the device-mapped model-step buffer failed");
  if (h->cfg.save_samples)
    MPPI_TRY(allocZeroed(h, h->samples_d, (size_t)D * K * T * C, "samples_d"));
  if (h->rows_in_hbm)
  {
    MPPI_TRY(allocZeroed(h, h->rows_d, h->model->globalRowsFloats(h->num_blocks, h->bx * h->bz, T), "rows_d"));
    h->model->setGlobalRows(h->rows_d);
  }
  return MPPI_OK;
}

/** the finalize kernels' scratch at long horizons, and the split hand-over's carry blocks and side stream */
static mppi_status allocFinalize(mppi_handle h, const CreateSwitches& sw)
{
  const mppi_config& cfg = h->cfg;
  const int T = cfg.num_timesteps, D = h->D, C = h->C;
  // the finalize kernels keep the control sequence twice in LDS (smoothing buffer + result) while that is a minor share of
  // it; beyond 64 KiB per system (T * C > ~8 000) — or on request (test hook) — both live in HBM
  const size_t per_sys = kernels::finalizeScratchFloats(T, C);
  if (per_sys * sizeof(float) > 64 * 1024 || sw.finalize_scratch)
    MPPI_TRY(allocZeroed(h, h->fin_scratch_d, (size_t)D * per_sys, "fin_scratch_d"));
  // split hand-over (mppi_handle_s::split_finalize): Vanilla / Colored / Tube handles on the low-latency path
  // (not on a caller's stream: there a stream synchronisation is the caller's way to wait for everything the library launched)
  if (h->low_latency && h->stream.owned() && cfg.world_size == 1 && !cfg.force_exchange && !sw.no_split_finalize &&
      (((cfg.controller == MPPI_CONTROLLER_VANILLA || cfg.controller == MPPI_CONTROLLER_COLORED) && D == 1) ||
       (cfg.controller == MPPI_CONTROLLER_TUBE && D == 2)))
  {
    MPPI_TRY(allocZeroed(h, h->carry_d, 2 * h->in_floats + 4, "carry_d"));  // two carry blocks + their ready words (one per system)
    if (hipMemsetAsync(h->carry_d, 0, sizeof(float) * (2 * h->in_floats + 4), h->stream) != hipSuccess)
      return fail(nullptr, MPPI_ERR_HIP, "mppi_create: clearing the carry blocks");
    if (h->fin_scratch_d)
      MPPI_TRY(allocZeroed(h, h->fin_scratch2_d, (size_t)D * per_sys, "fin_scratch2_d"));
    if (h->side_stream.create(hipStreamNonBlocking) != hipSuccess || h->ev_side.create(hipEventDisableTiming) != hipSuccess)
      return fail(nullptr, MPPI_ERR_HIP, "mppi_create: side stream of the split hand-over");
    h->split_finalize = true;
  }
  return MPPI_OK;
}

/** the host's sequences, and which of them is system z of the kernels */
static void wireSystemTable(mppi_handle h)
{
  const int T = h->cfg.num_timesteps, S = h->S, C = h->C;
  h->control_h.assign((size_t)T * C, 0.0f);
  h->history_h.assign((size_t)2 * C, 0.0f);
  h->state_h.assign((size_t)T * S, 0.0f);
  h->nominal_control_h.assign((size_t)T * C, 0.0f);
  h->nominal_state_h.assign((size_t)T * S, 0.0f);
  h->tube_x_h.assign((size_t)S, 0.0f);
  h->slide_scale_h.assign(C, 0.0f);  // controller.cuh:67 slide_control_scale_ = Zero()
  h->nominal_history_h.assign((size_t)2 * C, 0.0f);
  h->rm_nominal_state.assign(S, 0.0f);
  SystemTable& t = h->sys;
  const int real = h->cfg.controller == MPPI_CONTROLLER_ROBUST ? 1 : 0;  // Robust MPPI: system 0 is the nominal one
  t.control[real] = &h->control_h;
  t.state[real] = &h->state_h;
  t.history[real] = &h->history_h;
  t.stats[real] = &h->stats_h.real_sys;
  if (h->D == 2)
  {
    t.control[1 - real] = &h->nominal_control_h;
    t.state[1 - real] = &h->nominal_state_h;
    t.stats[1 - real] = &h->stats_h.nominal_sys;
    if (real)
    {  // ... which smooths with its own history and starts from the candidate chosen for it
      t.history[0] = &h->nominal_history_h;
      t.x0[0] = &h->rm_nominal_state;
    }
    else  // Tube: one history for both, the nominal system starts from its own state
      t.x0[1] = &h->tube_x_h;
  }
}

/** MPPI_AMD_REDUCTION=reference | reference_fma: every handle of the process starts in the reference-order reduction */
static mppi_status startReductionMode(mppi_handle h, const char* red)
{
  if (!red || !red[0] || exchangeActive(h))
    return MPPI_OK;
  const int mode = !strcmp(red, "reference") ? MPPI_REDUCTION_REFERENCE_ORDER :
                   !strcmp(red, "reference_fma") ? MPPI_REDUCTION_REFERENCE_ORDER_FMA : MPPI_REDUCTION_FUSED;
  if (mode == MPPI_REDUCTION_FUSED)
    return MPPI_OK;
  h->reduction_mode = mode;
  // ensureExactBuffers reports to the handle, which is about to go: the text moves to mppi_last_error(NULL)
  return ensureExactBuffers(h) == MPPI_OK ? MPPI_OK : fail(nullptr, MPPI_ERR_HIP, h->last_error);
}

mppi_status mppi_create(const mppi_config* cfg, mppi_handle* out)
{
  if (!cfg)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: null argument");
  return mppi_create_with_sampler(cfg, plan::defaultSampler(cfg->controller), out);
}

mppi_status mppi_create_with_sampler(const mppi_config* cfg, int sampler_kind, mppi_handle* out)
{
  MPPI_TRY(checkArguments(cfg, sampler_kind, out));
  MPPI_TRY(checkDevice(*cfg));
  const CreateSwitches sw{};

  std::unique_ptr<mppi_handle_s> owner(new mppi_handle_s());
  mppi_handle h = owner.get();
  h->cfg = *cfg;
  h->cfg.world_size = cfg->world_size > 0 ? cfg->world_size : 1;
  h->model_name = cfg->model;
  h->cfg.model = h->model_name.c_str();
  h->sampler_kind = sampler_kind;
  MPPI_TRY(resolveModel(h->cfg, h->model_name, sampler_kind, h->model));

  LaunchPlan plan;
  std::string refusal;
  const mppi_status planned = planLaunch(h->cfg, sampler_kind, *h->model, sw.rows_in_hbm, &plan, &refusal);
  if (planned != MPPI_OK)
    return fail(nullptr, planned, refusal);
  h->D = plan.D;
  h->bx = plan.bx;
  h->by = plan.by;
  h->bz = plan.bz;
  h->pipeline = plan.pipeline;
  h->rm_pipeline = plan.rm_pipeline;
  h->rows_in_hbm = plan.rows_in_hbm;  // the model's row pointer stays null until allocWorkBuffers has the buffer
  h->S = h->model->S;
  h->C = h->model->C;
  h->O = h->model->O;
  h->K_local = cfg->num_rollouts / h->cfg.world_size;
  h->K_offset = cfg->rank * h->K_local;
  h->num_blocks = (h->K_local + h->bx - 1) / h->bx;
  h->TC = cfg->num_timesteps * h->C;
  h->PS = kernels::partialStride(cfg->num_timesteps, h->C);
  h->noise_source = cfg->noise_source;
  h->noise_floats = h->model->noiseFloatsPerRollout(cfg->num_timesteps);
  if (h->noise_source < 0 || h->noise_source > MPPI_NOISE_ROCRAND_HOST)
    return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_create: unknown noise_source");

  HIP_TRY(nullptr, hipSetDevice(cfg->device));
  if (cfg->stream)
    h->stream.adopt((hipStream_t)cfg->stream);
  else
    HIP_TRY(nullptr, h->stream.create(hipStreamNonBlocking));
  h->stream_merge_enabled = !sw.no_stream_merge;
  h->merge_control_enabled = !sw.no_merge_control;
  MPPI_TRY(allocHandOver(h, sw));
  MPPI_TRY(allocWorkBuffers(h));
  MPPI_TRY(allocFinalize(h, sw));
  {
    hipError_t e = h->ev_a.create(hipEventDefault);
    if (e == hipSuccess)
      e = h->ev_b.create(hipEventDefault);
    if (e == hipSuccess)
      e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
      return fail(nullptr, MPPI_ERR_HIP, std::string("mppi_create: event / stream setup: ") + hipGetErrorString(e));
  }
  wireSystemTable(h);
  MPPI_TRY(startReductionMode(h, sw.reduction));
  *out = owner.release();
  return MPPI_OK;
}
