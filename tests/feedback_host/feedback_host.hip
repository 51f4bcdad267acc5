/**
 * feedback_host.hip — the HOST build of the DDP backward pass (include/mppi_amd/feedback_controllers/ddp_backward.hpp), exported
 * for ctypes.  TEST CODE ONLY.  Compiled by tests/feedback_host/__init__.py with hipcc for the host alone;
 * tests/test_feedback.py holds it to a float64 restatement of the reference's ddp.h, tests/test_feedback_gpu.py holds
 * ddpBackwardKernel (the device build of the same header) to it bit for bit.
 */
#include "mppi_amd/feedback_controllers/ddp_backward.hpp"

extern "C" {
/** dims = S * 100 + C of one of the shipped models with computeGrad: 401 cartpole, 402 double integrator, 702 RacerDubins /
 *  AutoRally network, 1304 quadrotor.  A[T][S][S], B[T][S][C], Q[S][S], R[C][C], Qf[S][S] -> gains[T][S][C].
 *  Returns 1 (done, *fail_step = -1), 0 (step *fail_step failed) or -1 (dims unknown, nothing touched). */
int feedback_host_backward(int dims, const float* A, const float* B, const float* Q, const float* R, const float* Qf, float dt,
                           int T, float* gains, int* fail_step)
{
  switch (dims)
  {
    case 401:
      return mppi::ddp::backwardPass<4, 1>(A, B, Q, R, Qf, dt, T, gains, fail_step) ? 1 : 0;
    case 402:
      return mppi::ddp::backwardPass<4, 2>(A, B, Q, R, Qf, dt, T, gains, fail_step) ? 1 : 0;
    case 702:
      return mppi::ddp::backwardPass<7, 2>(A, B, Q, R, Qf, dt, T, gains, fail_step) ? 1 : 0;
    case 1304:
      return mppi::ddp::backwardPass<13, 4>(A, B, Q, R, Qf, dt, T, gains, fail_step) ? 1 : 0;
  }
  return -1;
}
}  // extern "C"
