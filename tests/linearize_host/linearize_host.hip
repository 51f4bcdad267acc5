/**
 * linearize_host.hip — the HOST forms of the shipped computeGrad methods (__host__ __device__ in the model headers), exported for
 * ctypes.  TEST CODE ONLY.  Compiled by tests/linearize_host/__init__.py with hipcc for the host alone; tests/test_linearize.py
 * holds them to float64 restatements, tests/test_linearize_gpu.py holds the device build of the same headers to them bit for bit.
 */
#include "mppi_amd/dynamics/cartpole/cartpole_dynamics.hpp"
#include "mppi_amd/dynamics/double_integrator/di_dynamics.hpp"
#include "mppi_amd/dynamics/racer_dubins/racer_dubins.hpp"
#include "mppi_amd/dynamics/racer_dubins/racer_dubins_elevation.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#include "mppi_amd/dynamics/autorally/ar_nn_model.hpp"
#include "mppi_amd/dynamics/bicycle_slip/bicycle_slip_lstm.hpp"

#include <cstring>

namespace
{
/** what the engine does around the call: cleared storage, then the model's method */
template <class DYN_T, class... SHARED>
int evalAll(DYN_T& dyn, const float* x, const float* u, int n, float* A, float* B, int* returned, SHARED... shared)
{
  constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM;
  memset(A, 0, sizeof(float) * n * S * S);
  memset(B, 0, sizeof(float) * n * S * C);
  int all = 1;
  for (int p = 0; p < n; p++)
    all &= dyn.computeGrad(x + p * S, u + p * C, A + p * S * S, B + p * S * C, shared...) ? 1 : 0;
  *returned = all;
  return S * 100 + C;
}
}  // namespace

extern "C" {
/** model: 0 cartpole (params: cart mass, pole mass, pole length), 1 double integrator, 2 RacerDubins (default parameters),
 *  3 quadrotor (params: tau_roll, tau_pitch, tau_yaw, mass), 4 NeuralNetModel<7,2,3> (weights: the 1412-float blob).
 *  Returns S * 100 + C, -1 for an unknown model; *returned: the AND of the method's return values. */
int linearize_host_eval(int model, const float* params, const float* weights, const float* x, const float* u, int n, float* A,
                        float* B, int* returned)
{
  switch (model)
  {
    case 0:
    {
      CartpoleDynamics d(params[0], params[1], params[2]);
      return evalAll(d, x, u, n, A, B, returned);
    }
    case 1:
    {
      DoubleIntegratorDynamics d;
      return evalAll(d, x, u, n, A, B, returned);
    }
    case 2:
    {
      RacerDubins d;
      return evalAll(d, x, u, n, A, B, returned);
    }
    case 3:
    {
      QuadrotorDynamics d;
      d.params_.tau_roll = params[0];
      d.params_.tau_pitch = params[1];
      d.params_.tau_yaw = params[2];
      d.params_.mass = params[3];
      return evalAll(d, x, u, n, A, B, returned);
    }
    case 4:
    {
      NeuralNetModel<7, 2, 3> d;
      return evalAll(d, x, u, n, A, B, returned, const_cast<float*>(weights));
    }
  }
  return -1;
}
/** bit i: class i of the list below declares computeGrad (plugin/dynamics.hpp: has_compute_grad); bit 16 + i: in the
 *  wave-per-point form.  0 cartpole, 1 double integrator, 2 RacerDubins, 3 quadrotor, 4 NeuralNetModel, 5 NeuralNetModelMFMA,
 *  6 NeuralNetModelWave, 7 RacerDubinsElevation, 8 BicycleSlipLSTM */
unsigned linearize_host_traits()
{
  unsigned bits = 0;
  int i = 0;
  auto add = [&](bool has, bool wave) {
    bits |= (has ? 1u : 0u) << i | (wave ? 1u : 0u) << (16 + i);
    i++;
  };
#define CLASS_BITS(T) add(mppi::has_compute_grad<T>::value, mppi::compute_grad_wave<T>::value)
  CLASS_BITS(CartpoleDynamics);
  CLASS_BITS(DoubleIntegratorDynamics);
  CLASS_BITS(RacerDubins);
  CLASS_BITS(QuadrotorDynamics);
  using NN = NeuralNetModel<7, 2, 3>;
  using NN_MFMA = NeuralNetModelMFMA<7, 2, 3>;
  using NN_WAVE = NeuralNetModelWave<7, 2, 3>;
  CLASS_BITS(NN);
  CLASS_BITS(NN_MFMA);
  CLASS_BITS(NN_WAVE);
  CLASS_BITS(RacerDubinsElevation);
  CLASS_BITS(BicycleSlipLSTM);
#undef CLASS_BITS
  return bits;
}
}  // extern "C"
