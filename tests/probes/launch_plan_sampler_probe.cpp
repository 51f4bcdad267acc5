/**
 * launch_plan_sampler_probe.cpp — TEST CODE: planLaunch with the sampler kind named (mppi-generic_amd/csrc/launch_plan.hpp) and the
 * rule of mppi_set_independent_noise, against a stub model, host only, no device and no engine library.  The companion of
 * launch_plan_probe.cpp (whose cases run with each controller's own sampler); same case lines, read from stdin, with
 *   sampler=<mppi_sampler_kind>      the sampler kind of the model instantiation (default 0)
 *   indep=1                          ask plan::independentNoiseRule(ctl, sampler) instead of the plan
 * Model keys: shapes= default= pipeline= fold= hbm= c= base= ring=;  request keys: ctl= bx= by= variant= T= forced=.
 * The stub's LDS request is linear: base + slots * T * c * 4 (+ ring when pipelined), slots = bx * bz; the row term is dropped
 * while the row pointer is set.  Prints per case
 *   ok D bx by bz pipeline rm_pipeline rows_in_hbm lds rows=<null|set>
 *   refused <status> rows=<null|set> <text>
 *   indep-ok   |   indep-refused <status> <text>
 * tests/test_colored_tube_plan.py holds the expectations.
 */
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "launch_plan.hpp"

using namespace mppi::engine;
namespace kernels = mppi::kernels;

struct StubModel : ModelBase
{
  std::vector<int> shapes;
  bool pipeline = false, fold = false, hbm = false;
  size_t c = 1, base = 0, ring = 0;
  float* rows = nullptr;

  size_t rowBytes(int slots, int T) const
  {
    return rows ? 0 : (size_t)slots * T * c * 4;
  }

  /* what the plan asks */
  bool supportsShape(int bx, int by, int bz) const override
  {
    for (size_t i = 0; i + 2 < shapes.size(); i += 3)
      if (shapes[i] == bx && shapes[i + 1] == by && shapes[i + 2] == bz)
        return true;
    return false;
  }
  void listShapes(std::vector<int>& out) const override { out.insert(out.end(), shapes.begin(), shapes.end()); }
  void listReplicatedLaneShapes(std::vector<int>&) const override {}
  bool supportsPipeline() const override { return pipeline; }
  bool supportsPipelineFold(int bx, int by, int bz) const override { return fold && bx == 32 && by == 1 && bz == 2; }
  bool supportsPipelineRep(int, int, int) const override { return false; }
  bool supportsRMPPI() const override { return true; }
  bool supportsRMPPIPipeline() const override { return false; }
  size_t globalRowsFloats(int blocks, int slots, int T) const override { return hbm ? (size_t)blocks * slots * T * c : 0; }
  void setGlobalRows(float* rows_d) override { rows = rows_d; }
  size_t rolloutSharedBytes(int bx, int, int bz, int T, int, bool pipelined) override
  {
    return base + (pipelined ? ring : 0) + rowBytes(bx * bz, T);
  }
  size_t rmppiSharedBytes(int bx, int T) override { return base + rowBytes(bx * 2, T); }
  size_t rmppiPipelineSharedBytes(int) override { return 0; }

  /* what it never calls */
  mppi_status setDynamicsParams(const void*, size_t) override { return MPPI_ERR_STATE; }
  mppi_status setCostParams(const void*, size_t) override { return MPPI_ERR_STATE; }
  void setControlRanges(const float*) override {}
  void setControlDeadband(const float*) override {}
  void getZeroControl(float*) const override {}
  bool hostEnforceConstraints(float*) const override { return true; }
  void setSamplerParams(const mppi_gaussian_params*, int) override {}
  void setTimeSpecificStdDev(const float*) override {}
  size_t noiseFloatsPerRollout(int T) const override { return (size_t)T * c; }
  mppi_status launchNoiseDump(const SamplerLaunchState&, float*, hipStream_t, std::string&) override { return MPPI_ERR_STATE; }
  mppi_status launchRollout(int, int, int, bool, const kernels::RolloutArgs&, const SamplerLaunchState&, hipStream_t,
                            std::string&) override { return MPPI_ERR_STATE; }
  mppi_status launchFinalize(int, const kernels::FinalizeArgs&, hipStream_t, std::string&) override { return MPPI_ERR_STATE; }
  mppi_status launchModelStep(float*, float*, float, int, hipStream_t, std::string&) override { return MPPI_ERR_STATE; }
};

/** "64x1x1,16x4x1" -> flat triples; "64x1" -> a pair */
static std::vector<int> numbers(const std::string& s)
{
  std::vector<int> out;
  std::string cur;
  for (char ch : s + ",")
  {
    if (ch == 'x' || ch == ',')
    {
      if (!cur.empty())
        out.push_back(atoi(cur.c_str()));
      cur.clear();
    }
    else
      cur += ch;
  }
  return out;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line))
  {
    if (line.empty() || line[0] == '#')
      continue;
    StubModel m;
    mppi_config cfg{};
    cfg.model = "stub";
    bool forced = false, indep = false;
    int sampler = MPPI_SAMPLER_GAUSSIAN;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok)
    {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos)
      {
        fprintf(stderr, "launch_plan_sampler_probe: token without '=': %s\n", tok.c_str());
        return 2;
      }
      const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
      const long n = atol(v.c_str());
      if (k == "shapes") m.shapes = numbers(v);
      else if (k == "default") { const std::vector<int> d = numbers(v); m.default_bx = d.at(0); m.default_by = d.at(1); }
      else if (k == "pipeline") m.pipeline = n != 0;
      else if (k == "fold") m.fold = n != 0;
      else if (k == "hbm") m.hbm = n != 0;
      else if (k == "c") m.c = (size_t)n;
      else if (k == "base") m.base = (size_t)n;
      else if (k == "ring") m.ring = (size_t)n;
      else if (k == "ctl") cfg.controller = (int)n;
      else if (k == "sampler") sampler = (int)n;
      else if (k == "indep") indep = n != 0;
      else if (k == "bx") cfg.block_x = (int)n;
      else if (k == "by") cfg.block_y = (int)n;
      else if (k == "variant") cfg.kernel_variant = (int)n;
      else if (k == "T") cfg.num_timesteps = (int)n;
      else if (k == "forced") forced = n != 0;
      else
      {
        fprintf(stderr, "launch_plan_sampler_probe: unknown key %s\n", k.c_str());
        return 2;
      }
    }
    std::string err;
    if (indep)
    {
      const mppi_status st = plan::independentNoiseRule(cfg.controller, sampler, &err);
      if (st == MPPI_OK)
        printf("indep-ok\n");
      else
        printf("indep-refused %d %s\n", (int)st, err.c_str());
      continue;
    }
    LaunchPlan p;
    const mppi_status st = planLaunch(cfg, sampler, m, forced, &p, &err);
    const char* rows = m.rows ? "set" : "null";
    if (st == MPPI_OK)
      printf("ok %d %d %d %d %d %d %d %zu rows=%s\n", p.D, p.bx, p.by, p.bz, (int)p.pipeline, (int)p.rm_pipeline,
             (int)p.rows_in_hbm, p.lds, rows);
    else
      printf("refused %d rows=%s %s\n", (int)st, rows, err.c_str());
  }
  return 0;
}
