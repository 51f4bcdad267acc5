/**
 * launch_plan_probe.cpp — TEST CODE: planLaunch (mppi-generic_amd/csrc/launch_plan.hpp) against a stub model, host only, no
 * device and no engine library.  Reads one case per line from stdin, `key=value` tokens separated by blanks:
 *   model:   shapes=64x1x1,16x4x1,...  (registered shapes in listing order)   rep=64x4x1,...  (the replicated-lane ones among them)
 *            default=64x1  pipeline=0|1  fold=0|1  piperep=0|1  rmppi=0|1  hbm=0|1  (globalRowsFloats > 0)
 *            c=<channels>  base=<bytes>  ring=<bytes>  rmpipe=<bytes, 0: no pipelined Robust kernel>
 *   request: ctl=<mppi_controller_kind>  bx=  by=  variant=<mppi_kernel_variant>  T=  forced=0|1
 * The stub's LDS request is linear:  base + slots * T * c * 4  (+ ring when pipelined), slots = bx * bz; the row term
 * slots * T * c * 4 is dropped while the row pointer is set, as the samplers do.  Prints per case
 *   ok D bx by bz pipeline rm_pipeline rows_in_hbm lds rows=<null|set>
 *   refused <status> rows=<null|set> <text>
 * where rows= is the stub's row pointer after the call.  tests/test_launch_plan.py holds the expectations.
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
  std::vector<int> shapes, rep;
  bool pipeline = false, fold = false, piperep = false, rmppi = false, hbm = false;
  size_t c = 1, base = 0, ring = 0, rmpipe = 0;
  float* rows = nullptr;

  static bool has(const std::vector<int>& l, int bx, int by, int bz)
  {
    for (size_t i = 0; i + 2 < l.size(); i += 3)
      if (l[i] == bx && l[i + 1] == by && l[i + 2] == bz)
        return true;
    return false;
  }
  size_t rowBytes(int slots, int T) const
  {
    return rows ? 0 : (size_t)slots * T * c * 4;
  }

  /* what the plan asks */
  bool supportsShape(int bx, int by, int bz) const override { return has(shapes, bx, by, bz); }
  void listShapes(std::vector<int>& out) const override { out.insert(out.end(), shapes.begin(), shapes.end()); }
  void listReplicatedLaneShapes(std::vector<int>& out) const override { out.insert(out.end(), rep.begin(), rep.end()); }
  bool supportsPipeline() const override { return pipeline; }
  bool supportsPipelineFold(int bx, int by, int bz) const override { return fold && bx == 32 && by == 1 && bz == 2; }
  bool supportsPipelineRep(int bx, int by, int bz) const override { return piperep && bz == 1 && has(rep, bx, by, bz); }
  bool supportsRMPPI() const override { return rmppi; }
  bool supportsRMPPIPipeline() const override { return rmpipe > 0; }
  size_t globalRowsFloats(int blocks, int slots, int T) const override { return hbm ? (size_t)blocks * slots * T * c : 0; }
  void setGlobalRows(float* rows_d) override { rows = rows_d; }
  size_t rolloutSharedBytes(int bx, int, int bz, int T, int, bool pipelined) override
  {
    return base + (pipelined ? ring : 0) + rowBytes(bx * bz, T);
  }
  size_t rmppiSharedBytes(int bx, int T) override { return base + rowBytes(bx * 2, T); }
  size_t rmppiPipelineSharedBytes(int T) override { return rmpipe ? rmpipe + rowBytes(64 * 2, T) : 0; }

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
    bool forced = false;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok)
    {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos)
      {
        fprintf(stderr, "launch_plan_probe: token without '=': %s\n", tok.c_str());
        return 2;
      }
      const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
      const long n = atol(v.c_str());
      if (k == "shapes") m.shapes = numbers(v);
      else if (k == "rep") m.rep = numbers(v);
      else if (k == "default") { const std::vector<int> d = numbers(v); m.default_bx = d.at(0); m.default_by = d.at(1); }
      else if (k == "pipeline") m.pipeline = n != 0;
      else if (k == "fold") m.fold = n != 0;
      else if (k == "piperep") m.piperep = n != 0;
      else if (k == "rmppi") m.rmppi = n != 0;
      else if (k == "hbm") m.hbm = n != 0;
      else if (k == "c") m.c = (size_t)n;
      else if (k == "base") m.base = (size_t)n;
      else if (k == "ring") m.ring = (size_t)n;
      else if (k == "rmpipe") m.rmpipe = (size_t)n;
      else if (k == "ctl") cfg.controller = (int)n;
      else if (k == "bx") cfg.block_x = (int)n;
      else if (k == "by") cfg.block_y = (int)n;
      else if (k == "variant") cfg.kernel_variant = (int)n;
      else if (k == "T") cfg.num_timesteps = (int)n;
      else if (k == "forced") forced = n != 0;
      else
      {
        fprintf(stderr, "launch_plan_probe: unknown key %s\n", k.c_str());
        return 2;
      }
    }
    LaunchPlan p;
    std::string err;
    const mppi_status st = planLaunch(cfg, m, forced, &p, &err);
    const char* rows = m.rows ? "set" : "null";
    if (st == MPPI_OK)
      printf("ok %d %d %d %d %d %d %d %zu rows=%s\n", p.D, p.bx, p.by, p.bz, (int)p.pipeline, (int)p.rm_pipeline,
             (int)p.rows_in_hbm, p.lds, rows);
    else
      printf("refused %d rows=%s %s\n", (int)st, rows, err.c_str());
  }
  return 0;
}
