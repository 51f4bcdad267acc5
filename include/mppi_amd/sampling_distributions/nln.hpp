/**
 * nln.hpp — NLNDistribution sampler plugin (normal–log-normal noise, the log-MPPI sampler), MI355X design.
 *
 * Replaces (reference paths relative to include/mppi/sampling_distributions/):
 *   NLNDistributionImpl::generateSamples      nln/nln.cu:88-142   (curandGenerateNormal, curandGenerateLogNormal per control,
 *                                                                  the element-wise product, then setGaussianControls)
 * Reference data flow per iteration: cuRAND fills a normal tensor [K][T][C] and, control by control, a log-normal tensor
 * exp(sigma_c z') with mean 0 and std_dev = params_.std_dev[c] (nln.cu:106-121); a kernel multiplies the two in place
 * (:123-130) and setGaussianControls rewrites the product as v = mu + sigma * eps' — three more passes over V than the
 * Gaussian sampler's.
 *
 * Here the product never exists in memory.  Row element e = t * C + c of global rollout k, noise stream s (0, or the
 * distribution index when use_same_noise_for_all_distributions is off):
 *     z1   = normal4(seed, generation, s,                   k, e >> 2)[e & 3]
 *     z2   = normal4(seed, generation, NLN_STREAM_BASE + s, k, e >> 2)[e & 3]
 *     eps' = z1 * det::exp(params_.std_dev[c] * z2)          (three rounded fp32 operations: product, exp, product)
 * The log-normal's sigma is distribution 0's, undecayed, and never the time-specific table — what the reference hands to
 * curandGenerateLogNormal.  Everything downstream of eps' (decayed / time-specific sigma, the special-trajectory rules,
 * clamping, write-back, the likelihood-ratio cost, the weighted reduction) is GaussianDistribution's code, unchanged.
 *
 * The three places the parent produces eps are shadowed (the kernels call them through the concrete sampler type, so the
 * Gaussian instantiations compile to what they compiled to before):
 *   drawQuad()                  the in-loop draw: two Philox quads and four det::exp per four row elements, independent of
 *                               the state — work for the sampler waves of the role-pipelined kernels;
 *   initializeDistributions()   the row pre-fill (blockDim.y > 1, replicated-lane kernels);
 *   sampleAt()                  random access (Robust MPPI's candidate evaluation); the QuadCache holds the combined quad.
 * Injected noise (NOISE_EPS_BUFFER) is taken as eps' itself and is not multiplied again.
 */
#ifndef MPPI_AMD_NLN_DISTRIBUTION_HPP_
#define MPPI_AMD_NLN_DISTRIBUTION_HPP_

#include "mppi_amd/det_math.h"
#include "mppi_amd/sampling_distributions/gaussian.hpp"

namespace mppi
{
namespace sampling_distributions
{
/** Philox stream of the log-normal factor's exponent: NLN_STREAM_BASE + the noise stream of the normal factor.  Streams 0..1
 *  are the Gaussian distributions, 1 + c the colored-noise spectrum of control c. */
static constexpr unsigned NLN_STREAM_BASE = 16u;

template <class DYN_PARAMS_T>
class NLNDistribution : public GaussianDistribution<DYN_PARAMS_T>
{
public:
  using PARENT = GaussianDistribution<DYN_PARAMS_T>;
  /** declared here, not inherited: the shadowed draw methods below hold no block barrier either (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  static const int CONTROL_DIM = PARENT::CONTROL_DIM;
  typedef typename PARENT::SAMPLING_PARAMS_T SAMPLING_PARAMS_T;
  typedef typename PARENT::QuadCache QuadCache;
  static constexpr bool IN_LOOP_DRAW = true;
  static constexpr bool COLORED = false;
  static constexpr int SAMPLER_KIND = 2;  ///< MPPI_SAMPLER_NLN
  static constexpr bool SUPPORTS_GLOBAL_ROWS = true;

  NLNDistribution(hipStream_t stream = 0) : PARENT(stream)
  {
  }
  NLNDistribution(const SAMPLING_PARAMS_T& params, hipStream_t stream = 0) : PARENT(params, stream)
  {
  }

  /** sigma of the log-normal factor of element l of quad `quad`: params_.std_dev[(4 quad + l) % C].  Where C divides 4 the
   *  control index is a constant of the unrolled caller; otherwise the value is selected, never indexed (a run-time index
   *  into the kernel-argument copy of the object would move it to scratch memory). */
  __device__ inline float logNormalSigma(const int quad, const int l) const
  {
    if constexpr (4 % CONTROL_DIM == 0)
    {
      return this->params_.std_dev[l % CONTROL_DIM];
    }
    else
    {
      const int c = (4 * quad + l) % CONTROL_DIM;
      float s = this->params_.std_dev[0];
#pragma unroll
      for (int j = 1; j < CONTROL_DIM; j++)
        s = (c == j) ? this->params_.std_dev[j] : s;
      return s;
    }
  }

  /** eps' of row elements 4 quad .. 4 quad + 3 of GLOBAL rollout `rollout`, noise stream `stream` */
  __device__ __forceinline__ void nlnQuad(const unsigned stream, const uint32_t rollout, const int quad, float z[4]) const
  {
    float z1[4], z2[4];
    mppi::rng::normal4(this->seed_, this->generation_, stream, rollout, (uint32_t)quad, z1);
    mppi::rng::normal4(this->seed_, this->generation_, NLN_STREAM_BASE + stream, rollout, (uint32_t)quad, z2);
#pragma unroll
    for (int l = 0; l < 4; l++)
      z[l] = z1[l] * mppi::det::exp(logNormalSigma(quad, l) * z2[l]);
  }

  /** quad `quad` of local rollout `sample_index`, into registers (shadows GaussianDistribution::drawQuad) */
  __device__ __forceinline__ void drawQuad(const int sample_index, const int quad, float z[4]) const
  {
    nlnQuad(this->noise_stream_, (uint32_t)(sample_index + this->rollout_offset_), quad, z);
  }

  /** the row pre-fill (shadows GaussianDistribution::initializeDistributions): the parent's loop with the NLN quad; injected
   *  noise is eps' already and takes the parent's copy.  Forced inline: left to the inliner's size heuristic the body stays a
   *  function, and every rollout kernel that calls it then pays the call ABI (136 VGPRs, 200 B of scratch per lane). */
  __device__ __forceinline__ void initializeDistributions(const float* __restrict__ output, const float t_0, const float dt,
                                                 float* __restrict__ theta_d)
  {
    if (this->drawsInLoop())
      return;
    if (this->noise_source_ == NOISE_EPS_BUFFER)
    {
      PARENT::initializeDistributions(output, t_0, dt, theta_d);
      return;
    }
    const int TC = this->params_.num_timesteps * CONTROL_DIM;
    const int stride = this->rowStrideNow();
    const int bx = this->rolloutsPerBlock();
    const int tid_flat = (int)(threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z));
    const int nthreads = (int)(blockDim.x * blockDim.y * blockDim.z);
    const int row0 = (int)(blockIdx.x * bx);  // first local rollout of the block
    const int nrows = min(bx, this->params_.num_rollouts - row0);
    const int nz = this->systemsPerBlock();
    if (nrows <= 0)
      return;
    const int qpr = (TC + 3) >> 2;  // quads per row
    const int nquads = nrows * qpr;
    for (int i = tid_flat; i < nquads; i += nthreads)
    {
      const int row = i / qpr;
      const int q = i - row * qpr;
      for (int z = 0; z < (this->independentNoise() ? nz : 1); z++)
      {
        float zn[4];
        nlnQuad((unsigned)z, (uint32_t)(row0 + row + this->rollout_offset_), q, zn);
#pragma unroll
        for (int l = 0; l < 4; l++)
        {
          const int col = q * 4 + l;
          if (col < TC)
          {
            if (this->independentNoise())
              theta_d[(z * bx + row) * stride + col] = zn[l];
            else
              for (int zz = 0; zz < nz; zz++)
                theta_d[(zz * bx + row) * stride + col] = zn[l];
          }
        }
      }
    }
  }

  /** random access to one shaped sample (shadows GaussianDistribution::sampleAt); the cache holds the COMBINED quad */
  __device__ __forceinline__ void sampleAt(const int sample_index, const int t, const int distribution_index,
                                  float* __restrict__ control, QuadCache* cache = nullptr) const
  {
    const int d = distribution_index >= this->params_.num_distributions ? 0 : distribution_index;
    const float* mean = this->control_means_d_ + (size_t)(this->params_.num_timesteps * d + t) * CONTROL_DIM;
    const bool use_mean = ((sample_index + this->rollout_offset_) == 0) || (t < this->optimization_stride_);
    const bool pure = this->isPureNoise(sample_index);
    QuadCache local;
    QuadCache& qc = cache ? *cache : local;
#pragma unroll
    for (int i = 0; i < CONTROL_DIM; i++)
    {
      const int e = t * CONTROL_DIM + i;
      float eps;
      if (this->noise_source_ == NOISE_EPS_BUFFER)
      {
        const size_t slab =
            this->independentNoise() ? (size_t)d * this->params_.num_rollouts * this->params_.num_timesteps * CONTROL_DIM : 0;
        eps = this->eps_d_[slab + (size_t)sample_index * this->params_.num_timesteps * CONTROL_DIM + e];
      }
      else
      {
        if ((e >> 2) != qc.quad)
        {  // (rows of one distribution and one rollout only: the cache is keyed by the quad index)
          qc.quad = e >> 2;
          nlnQuad(this->independentNoise() ? (unsigned)d : 0u, (uint32_t)(sample_index + this->rollout_offset_), e >> 2, qc.z);
        }
        eps = (e & 3) == 0 ? qc.z[0] : ((e & 3) == 1 ? qc.z[1] : ((e & 3) == 2 ? qc.z[2] : qc.z[3]));
      }
      control[i] = this->shapeSample(mean[i], this->template sigmaValue<false, true>(d, t, i), eps, use_mean, pure);
    }
  }
};

}  // namespace sampling_distributions
}  // namespace mppi

#endif
