/**
 * launch_plan.hpp — which rollout kernel a handle runs, decided once at mppi_create: block shape, fused or role-pipelined,
 * Robust MPPI's pipelined form, the Tube fold, the sample rows in LDS or in HBM, or the refusal.  Host only and pure: everything
 * planLaunch depends on is an argument (the configuration, the model's capability and LDS-size queries, MPPI_AMD_ROWS_IN_HBM as
 * `hbm_forced`); no environment, no handle, no HIP call.  tests/probes/launch_plan_probe.cpp runs it against a stub model.
 *
 * Precedence (DESIGN.md §2 has the table): Robust MPPI and the other controllers share nothing but the final LDS check, so
 * each has its own sequence of steps; a step takes what it names and returns a value, nothing is re-read after a later step
 * changed it.
 */
#ifndef MPPI_AMD_CSRC_LAUNCH_PLAN_HPP_
#define MPPI_AMD_CSRC_LAUNCH_PLAN_HPP_

#include <string>
#include <vector>

#include "mppi_amd.h"
#include "mppi_amd/engine/model_base.hpp"
#include "mppi_amd/engine/model_launch.hpp"  // MAX_LDS_BYTES

#pragma GCC visibility push(hidden)  // internal to the engine: nothing of it enters the library's export table
namespace mppi
{
namespace engine
{
struct LaunchPlan
{
  int D = 1, bx = 64, by = 1, bz = 1;
  bool pipeline = false;     ///< the role-pipelined rollout kernel (plain, folded or replicated-lane)
  bool rm_pipeline = false;  ///< Robust MPPI's role-pipelined kernel
  bool rows_in_hbm = false;  ///< the sampler's rows in HBM: mppi_create allocates them and calls setGlobalRows
  size_t lds = 0;            ///< the LDS request the plan was accepted with, in bytes
};

namespace plan
{
struct Block
{
  int bx, by;
};
/** one candidate: a block, the kernel kind, where the rows live, and the LDS request that combination makes */
struct Form
{
  Block block;
  bool pipeline, rows_in_hbm;
  size_t lds;
  bool fits() const
  {
    return lds <= MAX_LDS_BYTES;
  }
};

inline mppi_status refuse(std::string* err, mppi_status s, const std::string& msg)
{
  *err = msg;
  return s;
}

/* ---------------------------------------------------------------- which sampler a controller kind takes -------------- */
/** the sampler a controller kind runs with when none is named (mppi_create) */
inline int defaultSampler(int controller)
{
  return controller == MPPI_CONTROLLER_COLORED ? MPPI_SAMPLER_COLORED : MPPI_SAMPLER_GAUSSIAN;
}

/** the registry key mppi_create looks a model up under first: Tube with the colored sampler has registrations of its own
 *  (MPPI_SAMPLER_COLORED_TUBE), so that the ones under MPPI_SAMPLER_COLORED stay what MPPI_CONTROLLER_COLORED runs, one system */
inline int registrationKind(int controller, int sampler_kind)
{
  return controller == MPPI_CONTROLLER_TUBE && sampler_kind == MPPI_SAMPLER_COLORED ? MPPI_SAMPLER_COLORED_TUBE : sampler_kind;
}

/** Vanilla, Tube and Robust take the Gaussian or the NLN sampler, MPPI_CONTROLLER_COLORED the colored one — and so does Tube:
 *  the colored prologue writes one draw into the rows of both systems (the reference's use_same_noise_for_all_distributions).
 *  Robust MPPI evaluates its candidates with draws addressed one by one; the colored rows exist only as the result of a
 *  block-wide GEMM.  An unknown controller kind passes: the plan reports it. */
inline mppi_status samplerRule(int controller, int sampler_kind, std::string* err)
{
  const bool colored = sampler_kind == MPPI_SAMPLER_COLORED;
  if (controller == MPPI_CONTROLLER_TUBE && colored)
    return MPPI_OK;
  if (controller == MPPI_CONTROLLER_ROBUST && colored)
    return refuse(err, MPPI_ERR_UNSUPPORTED,
                  "mppi_create: Robust MPPI with MPPI_SAMPLER_COLORED is not available: its candidate evaluation draws single "
                  "samples by index (random access), the colored-noise rows come out of a block-wide GEMM prologue and have no "
                  "such draw");
  const bool ok = controller == MPPI_CONTROLLER_COLORED ? colored :
                                                          (sampler_kind == MPPI_SAMPLER_GAUSSIAN || sampler_kind == MPPI_SAMPLER_NLN);
  if (!ok)
    return refuse(err, MPPI_ERR_INVALID_ARG,
                  "mppi_create: the Vanilla, Tube and Robust controllers take MPPI_SAMPLER_GAUSSIAN or MPPI_SAMPLER_NLN, "
                  "MPPI_CONTROLLER_COLORED takes MPPI_SAMPLER_COLORED only");
  return MPPI_OK;
}

/** mppi_set_independent_noise(h, 1): the colored-noise sampler draws one spectrum per rollout, whatever the controller */
inline mppi_status independentNoiseRule(int controller, int sampler_kind, std::string* err)
{
  if (controller == MPPI_CONTROLLER_COLORED)
    return refuse(err, MPPI_ERR_UNSUPPORTED, "independent noise per distribution: the colored-noise sampler has one distribution");
  if (sampler_kind == MPPI_SAMPLER_COLORED)
    return refuse(err, MPPI_ERR_UNSUPPORTED,
                  "independent noise per distribution: the colored-noise sampler draws one spectrum per rollout for both systems "
                  "of a Tube handle; no per-system spectrum stream is assigned");
  return MPPI_OK;
}

/** an LDS-size query answered as if the sample rows were in HBM: the samplers drop their row term while their row pointer is
 *  set, so a placeholder stands in for the buffer mppi_create allocates later — for the length of the query only */
template <class F>
inline size_t ldsWithRowsInHbm(ModelBase& m, F sizeQuery)
{
  m.setGlobalRows(reinterpret_cast<float*>(16));
  const size_t bytes = sizeQuery();
  m.setGlobalRows(nullptr);
  return bytes;
}

inline bool hasHbmRows(const ModelBase& m, int T)
{
  return m.globalRowsFloats(1, 1, T) > 0;
}

/** the block the configuration asks for, the model's default where it leaves a dimension open */
inline Block requestedBlock(const mppi_config& cfg, const ModelBase& m)
{
  return { cfg.block_x > 0 ? cfg.block_x : m.default_bx, cfg.block_y > 0 ? cfg.block_y : m.default_by };
}
inline bool unshaped(const mppi_config& cfg)
{
  return cfg.block_x == 0 && cfg.block_y == 0;
}

/* ---------------------------------------------------------------- Robust MPPI ---------------------------------------- */
/** rmppiPipelineKernel applies: not refused by FUSED, block_x 0 or 64, a sampler with rows in HBM, and rings that fit */
inline bool robustPipelineFits(const mppi_config& cfg, ModelBase& m)
{
  if (cfg.kernel_variant == MPPI_KERNEL_FUSED || !(cfg.block_x == 0 || cfg.block_x == 64) || !hasHbmRows(m, cfg.num_timesteps))
    return false;
  const size_t need = ldsWithRowsInHbm(m, [&] { return m.rmppiPipelineSharedBytes(cfg.num_timesteps); });
  return need > 0 && need <= MAX_LDS_BYTES;
}

/** rolloutRMPPIKernel's block_x with the rows in LDS: the request, else 64, else 32 when the rows of 64 x 2 overflow */
inline int robustBlockX(const mppi_config& cfg, ModelBase& m)
{
  if (cfg.block_x != 0)
    return cfg.block_x;
  return m.rmppiSharedBytes(64, cfg.num_timesteps) > MAX_LDS_BYTES ? 32 : 64;
}

/** rolloutRMPPIKernel with the rows in HBM: at horizons whose rows of even 32 x 2 overflow the (64, 1, 2) block (or the
 *  requested one), on request the block the LDS form would have had.  Not accepted when even that overflows. */
inline Form robustRowsInHbm(const mppi_config& cfg, ModelBase& m, const Form& lds_form)
{
  const int bx = lds_form.fits() ? lds_form.block.bx : (cfg.block_x != 0 ? cfg.block_x : 64);
  const size_t lds = ldsWithRowsInHbm(m, [&] { return m.rmppiSharedBytes(bx, cfg.num_timesteps); });
  return { { bx, 1 }, false, lds <= MAX_LDS_BYTES, lds };
}

inline mppi_status planRobust(const mppi_config& cfg, ModelBase& m, bool hbm_forced, LaunchPlan* out, std::string* err)
{
  const int T = cfg.num_timesteps;
  if ((cfg.block_x != 0 && cfg.block_x != 64 && cfg.block_x != 32) || (cfg.block_y != 0 && cfg.block_y != 1))
    return refuse(err, MPPI_ERR_LAUNCH_SHAPE, "mppi_create: Robust MPPI runs with block shape (64, 1, 2) or (32, 1, 2)");
  out->rm_pipeline = robustPipelineFits(cfg, m);
  if (cfg.kernel_variant == MPPI_KERNEL_PIPELINE && !out->rm_pipeline)
    return refuse(err, MPPI_ERR_LAUNCH_SHAPE,
                  "mppi_create: the pipelined Robust MPPI kernel needs a model registered for it (replicated-lane MFMA / four-lane "
                  "dynamics, or a one-lane model registered with PIPELINE), the Gaussian sampler and block_x 0 or 64");
  Form f{};
  if (out->rm_pipeline)  // 64 rollouts x 2 systems, rows in HBM by design: the rings take their place in the LDS
    f = { { 64, 1 }, false, true, ldsWithRowsInHbm(m, [&] { return m.rmppiSharedBytes(64, T); }) };
  else
  {
    const int bx = robustBlockX(cfg, m);
    f = { { bx, 1 }, false, false, m.rmppiSharedBytes(bx, T) };
    if ((!f.fits() || hbm_forced) && hasHbmRows(m, T))
      f = robustRowsInHbm(cfg, m, f);
  }
  out->bx = f.block.bx;
  out->by = f.block.by;
  out->rows_in_hbm = f.rows_in_hbm;
  out->lds = f.lds;
  return MPPI_OK;
}

/* ---------------------------------------------------------------- Vanilla, Colored, Tube ----------------------------- */
/** the shape runs as a rollout kernel of the model: a registered shape, or — where the plan offers the role-pipelined forms
 *  (`offered`: pipelinedFormsOffered) — the folded pipeline's */
inline bool instantiated(const ModelBase& m, Block b, int bz, bool offered = true)
{
  return m.supportsShape(b.bx, b.by, bz) || (offered && m.supportsPipelineFold(b.bx, b.by, bz));
}

/** Tube with the colored-noise sampler runs the fused kernel only: no role-pipelined or folded kernel has been held to the
 *  oracle with the GEMM prologue filling the rows of two systems */
inline bool pipelinedFormsOffered(const mppi_config& cfg, int sampler_kind)
{
  return !(cfg.controller == MPPI_CONTROLLER_TUBE && sampler_kind == MPPI_SAMPLER_COLORED);
}

/** Tube with a fold-capable model, no shape requested and not FUSED: the two systems in the lanes of a wave, (32, 1, 2) */
inline bool tubeFolds(const mppi_config& cfg, ModelBase& m)
{
  return cfg.controller == MPPI_CONTROLLER_TUBE && unshaped(cfg) && cfg.kernel_variant != MPPI_KERNEL_FUSED &&
         m.supportsPipelineFold(32, 1, 2) && m.rolloutSharedBytes(32, 1, 2, cfg.num_timesteps, 2, true) <= MAX_LDS_BYTES;
}

/** no shape requested and the model's default has no instantiation for bz systems (a Tube controller on a model whose default
 *  exists for bz = 1 only): the registered shape for bz with the default's lanes per rollout if there is one, otherwise the
 *  first one listed (replicated-lane shapes come first); the default itself when nothing is registered for bz */
inline Block defaultBlockFor(const ModelBase& m, Block dflt, int bz, bool offered = true)
{
  if (instantiated(m, dflt, bz, offered))
    return dflt;
  std::vector<int> shapes;
  m.listShapes(shapes);
  int pick = -1;
  for (size_t i = 0; i + 2 < shapes.size(); i += 3)
  {
    if (shapes[i + 2] != bz)
      continue;
    if (pick < 0 || (shapes[i + 1] == dflt.by && shapes[pick + 1] != dflt.by))
      pick = (int)i;
  }
  return pick >= 0 ? Block{ shapes[pick], shapes[pick + 1] } : dflt;
}

/** a role-pipelined kernel exists for the block: plain (64, 1), folded, or replicated-lane */
inline bool pipelineEligible(const ModelBase& m, Block b, int bz)
{
  return (m.supportsPipeline() && b.bx == 64 && b.by == 1) || m.supportsPipelineFold(b.bx, b.by, bz) ||
         m.supportsPipelineRep(b.bx, b.by, bz);
}

/** the fused kernel with the rows in HBM (the reference's layout: no horizon limit).  At an overflow it runs on the block the
 *  configuration names (the fold and the bz default are undone), on request on the block chosen so far; a block without a
 *  fused instantiation leaves the form as it is.  Not accepted (rows_in_hbm false) when even that request overflows. */
inline Form fusedRowsInHbm(const mppi_config& cfg, ModelBase& m, const Form& f, int bz, int D)
{
  const Block b = f.fits() ? f.block : requestedBlock(cfg, m);
  if (!m.supportsShape(b.bx, b.by, bz))
    return f;
  const size_t lds = ldsWithRowsInHbm(m, [&] { return m.rolloutSharedBytes(b.bx, b.by, bz, cfg.num_timesteps, D, false); });
  return { b, false, lds <= MAX_LDS_BYTES, lds };
}

/** a sampler without rows in HBM at a long horizon: the registered shape for bz with the most rollouts per block whose rows
 *  fit the LDS, fused (the first listed among equals); `f` when none fits */
inline Form largestFittingShape(ModelBase& m, const Form& f, int bz, int T, int D)
{
  std::vector<int> shapes;
  m.listShapes(shapes);
  Form best = f;
  bool found = false;
  for (size_t i = 0; i + 2 < shapes.size(); i += 3)
  {
    if (shapes[i + 2] != bz)
      continue;
    const size_t need = m.rolloutSharedBytes(shapes[i], shapes[i + 1], bz, T, D, false);
    if (need <= MAX_LDS_BYTES && (!found || shapes[i] > best.block.bx))
    {
      best = { { shapes[i], shapes[i + 1] }, false, false, need };
      found = true;
    }
  }
  return best;
}

inline mppi_status planRollout(const mppi_config& cfg, ModelBase& m, bool hbm_forced, bool offered, LaunchPlan* out, std::string* err)
{
  const int T = cfg.num_timesteps, D = out->D, bz = out->bz;
  const Block block = offered && tubeFolds(cfg, m) ? Block{ 32, 1 } :
                      unshaped(cfg)                ? defaultBlockFor(m, requestedBlock(cfg, m), bz, offered) :
                                                     requestedBlock(cfg, m);
  if (!instantiated(m, block, bz, offered))
    return refuse(err, MPPI_ERR_LAUNCH_SHAPE,
                  "mppi_create: block shape (" + std::to_string(block.bx) + "," + std::to_string(block.by) + "," +
                      std::to_string(bz) + ") is not instantiated for model '" + cfg.model + "'");
  if (!offered && !(block.bx == 64 && block.by == 1))
    return refuse(err, MPPI_ERR_LAUNCH_SHAPE,
                  "mppi_create: the Tube controller with MPPI_SAMPLER_COLORED runs block shape (64,1,2) only — the one shape whose "
                  "prologue has been held to the oracle with two systems; (" + std::to_string(block.bx) + "," +
                      std::to_string(block.by) + "," + std::to_string(bz) + ") was asked for");
  if (cfg.kernel_variant == MPPI_KERNEL_PIPELINE && !offered)
    return refuse(err, MPPI_ERR_LAUNCH_SHAPE,
                  "mppi_create: the pipeline variant has no form for the Tube controller with MPPI_SAMPLER_COLORED; it runs the "
                  "fused kernel (MPPI_KERNEL_AUTO or MPPI_KERNEL_FUSED)");
  const bool pipe_ok = offered && pipelineEligible(m, block, bz);
  if (cfg.kernel_variant == MPPI_KERNEL_PIPELINE && !pipe_ok)
    return refuse(err, MPPI_ERR_LAUNCH_SHAPE,
                  "mppi_create: the pipeline variant needs a model registered for it and block shape (64, 1), or (64, REP, 1) "
                  "for replicated-lane (MFMA) dynamics");
  const auto rowsInLds = [&](bool pipeline) {
    return Form{ block, pipeline, false, m.rolloutSharedBytes(block.bx, block.by, bz, T, D, pipeline) };
  };
  Form f = rowsInLds(pipe_ok && cfg.kernel_variant != MPPI_KERNEL_FUSED);
  const bool hbm_rows = hasHbmRows(m, T);
  if (f.pipeline && (!f.fits() || hbm_forced) && hbm_rows)
  {  // the pipelined kernel keeps its block: rows in HBM, the output ring stays in the LDS
    const Form piped{ block, true, true,
                      ldsWithRowsInHbm(m, [&] { return m.rolloutSharedBytes(block.bx, block.by, bz, T, D, true); }) };
    if (piped.fits())
      f = piped;
  }
  if (!f.fits() && f.pipeline && cfg.kernel_variant == MPPI_KERNEL_AUTO)
    f = rowsInLds(false);  // the output ring does not fit next to the sample rows: the fused kernel
  if (!f.rows_in_hbm && (!f.fits() || hbm_forced) && cfg.kernel_variant != MPPI_KERNEL_PIPELINE && hbm_rows)
    f = fusedRowsInHbm(cfg, m, f, bz, D);
  if (!f.fits() && unshaped(cfg) && cfg.kernel_variant != MPPI_KERNEL_PIPELINE && offered)  // (Tube + colored keeps (64, 1, 2))
    f = largestFittingShape(m, f, bz, T, D);
  out->bx = f.block.bx;
  out->by = f.block.by;
  out->pipeline = f.pipeline;
  out->rows_in_hbm = f.rows_in_hbm;
  out->lds = f.lds;
  return MPPI_OK;
}
}  // namespace plan

/** The launch plan of a handle for the sampler kind of its model instantiation, or the refusal (status returned, text in *err;
 *  *out is unspecified then).  Leaves the model's row pointer null: mppi_create sets it once the buffer exists. */
inline mppi_status planLaunch(const mppi_config& cfg, int sampler_kind, ModelBase& model, bool hbm_forced, LaunchPlan* out,
                              std::string* err)
{
  *out = LaunchPlan();
  {
    const mppi_status rule = plan::samplerRule(cfg.controller, sampler_kind, err);
    if (rule != MPPI_OK)
      return rule;
  }
  const bool robust = cfg.controller == MPPI_CONTROLLER_ROBUST;
  switch (cfg.controller)
  {
    case MPPI_CONTROLLER_VANILLA:
    case MPPI_CONTROLLER_COLORED: out->D = 1; break;
    case MPPI_CONTROLLER_ROBUST:
      if (!model.supportsRMPPI())
        return plan::refuse(err, MPPI_ERR_UNSUPPORTED, std::string("mppi_create: model '") + cfg.model + "' is not instantiated for Robust MPPI");
      out->D = 2;
      break;
    case MPPI_CONTROLLER_TUBE: out->D = 2; break;
    default: return plan::refuse(err, MPPI_ERR_UNSUPPORTED, "mppi_create: controller kind not available in this build");
  }
  out->bz = out->D;
  // (Robust MPPI's two kernels are instantiated per model — checked above — not per block shape)
  const mppi_status st = robust ? plan::planRobust(cfg, model, hbm_forced, out, err) :
                                 plan::planRollout(cfg, model, hbm_forced, plan::pipelinedFormsOffered(cfg, sampler_kind), out, err);
  if (st != MPPI_OK)
    return st;
  if (out->lds > MAX_LDS_BYTES)
    return plan::refuse(err, MPPI_ERR_LDS_OVERFLOW,
                        "mppi_create: rollout kernel needs " + std::to_string(out->lds) + " B of LDS per block (max " +
                            std::to_string(MAX_LDS_BYTES) + ") — the sample rows of a block live in LDS and this sampler / "
                            "controller / kernel variant has no rows-in-HBM form; shorten the horizon or register a block shape "
                            "with fewer rollouts");
  return MPPI_OK;
}

/** ... with the sampler the controller kind runs with when none is named */
inline mppi_status planLaunch(const mppi_config& cfg, ModelBase& model, bool hbm_forced, LaunchPlan* out, std::string* err)
{
  return planLaunch(cfg, plan::defaultSampler(cfg.controller), model, hbm_forced, out, err);
}

}  // namespace engine
}  // namespace mppi
#pragma GCC visibility pop

#endif
