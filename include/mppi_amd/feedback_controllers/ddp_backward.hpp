/**
 * ddp_backward.hpp — the backward pass that produces the DDP tracking gains, stated once for host and device.
 *
 * reference: include/mppi/ddp/ddp.h:79-80 (Phi = I + A dt, Bd = B dt), :88-90 (boundary condition) and :95-124 (backward pass)
 * with the cost of DDPFeedback (TrackingCostDDP: d2L = blockdiag(Q, R), its off-diagonal block zero; TrackingTerminalCost: Qf).
 * With DDPParams::num_iterations = 1, the reference's default, the gains Lk_ are exactly one such pass: the forward pass and line
 * search behind it (:129-162) do not touch them.  Vx, lk, V are not computed, nothing here depends on them.
 *
 * Plain float arrays, row-major, templated on S (states) and C (controls), N = S + C:
 *   F  [S][N] = [Phi | Bd]     F(i, j) = fma(A(i, j), dt, i == j)  for j < S,   B(i, j - S) * dt  else
 *   W  [S][N] = Vxx F          W(i, j) = sum_l Vxx(i, l) F(l, j)
 *   Qm [N][N] = F^T W + blockdiag(Q, R) dt; rows r < S hold qxx (columns < S), rows r >= S hold [qux | quu]
 *   Lk [C][S] = -quu^-1 qux    column j: the unpivoted LDL^T of quu (lower triangle), forward, diagonal, backward substitution
 *   Vxx(i, j) <- 0.5 (vn(i, j) + vn(j, i)),  vn(i, j) = qxx(i, j) + sum_a qux(a, i) Lk(a, j)
 * for k = T - 2 ... 0, from Vxx = 0.5 (Qf + Qf^T); gains[k][i][a] = Lk(a, i) (DDPFeedbackState::fb_gain_traj_ order), row T - 1
 * zero (the reference's Lk_ is zero-initialised and never written there).
 *
 * THE ARITHMETIC IS FIXED HERE.  Every sum is one chain in ascending index order, each link a single det::fma (one rounding);
 * a chain starts from its additive term (Q(r, c) * dt, R * dt, qxx(i, j), the right-hand side) or from 0.0f; divisions are IEEE
 * `/`.  Every entry is a function of arrays complete before its phase, so WHO evaluates an entry — a host loop, or whichever
 * lane of ddpBackwardKernel (engine/feedback_kernel.hpp) — cannot change its bits: host build == device build, bit for bit
 * (tests/test_feedback_gpu.py).  Eigen's LDLT pivots, this one does not: equality with the reference's bits is not the aim,
 * tests/test_feedback.py bounds the distance to a float64 restatement of ddp.h.
 *
 * A pivot that is not > 0 or not finite fails the step (the reference exits the process there, ddp.h:115-119).
 */
#ifndef MPPI_AMD_DDP_BACKWARD_HPP_
#define MPPI_AMD_DDP_BACKWARD_HPP_

#include "mppi_amd/det_math.h"

namespace mppi
{
namespace ddp
{
/** entry (i, j) of F = [I + A dt | B dt] from `raw`, the entry of [A | B] at the same place */
template <int S>
MPPI_HD inline float fValue(const float raw, const float dt, const int i, const int j)
{
  if (j < S)
    return det::fma(raw, dt, i == j ? 1.0f : 0.0f);
  return raw * dt;
}

/** the same from A[S][S], B[S][C] */
template <int S, int C>
MPPI_HD inline float fEntry(const float* A, const float* B, const float dt, const int i, const int j)
{
  return fValue<S>(j < S ? A[i * S + j] : B[i * C + (j - S)], dt, i, j);
}

/** entry (i, j) of W = Vxx F */
template <int S, int C>
MPPI_HD inline float wEntry(const float* V, const float* F, const int i, const int j)
{
  constexpr int N = S + C;
  float acc = 0.0f;
#pragma unroll
  for (int l = 0; l < S; l++)
    acc = det::fma(V[i * S + l], F[l * N + j], acc);
  return acc;
}

/** the additive term of entry (r, c) of Qm: Q dt on the state block, R dt on the control block, 0 between them */
template <int S, int C>
MPPI_HD inline float costEntry(const float* Q, const float* R, const float dt, const int r, const int c)
{
  if (r < S && c < S)
    return Q[r * S + c] * dt;
  if (r >= S && c >= S)
    return R[(r - S) * C + (c - S)] * dt;
  return 0.0f;
}

/** entry (r, c) of Qm = F^T W + cost, `cost` = costEntry(r, c) */
template <int S, int C>
MPPI_HD inline float qEntry(const float* F, const float* W, const float cost, const int r, const int c)
{
  constexpr int N = S + C;
  float acc = cost;
#pragma unroll
  for (int l = 0; l < S; l++)
    acc = det::fma(F[l * N + r], W[l * N + c], acc);
  return acc;
}

/** the entries of Qm a step needs, numbered 0 ... S S + C N - 1: qxx row by row, then the rows [qux | quu] */
template <int S, int C>
MPPI_HD inline void qIndex(const int e, int& r, int& c)
{
  constexpr int N = S + C;
  if (e < S * S)
  {
    r = e / S;
    c = e - r * S;
  }
  else
  {
    const int f = e - S * S;
    r = S + f / N;
    c = f - (f / N) * N;
  }
}

/** unpivoted LDL^T of quu = Qm[S + a][S + b] (lower triangle read): unit lower L[C][C] (strict lower part written), d[C].
 *  false: a pivot is not > 0 or not finite. */
template <int S, int C>
MPPI_HD inline bool ldlt(const float* Qm, float* L, float* d)
{
  constexpr int N = S + C;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < C; j++)
  {
    float s = Qm[(S + j) * N + S + j];
#pragma unroll
    for (int k = 0; k < j; k++)
      s = det::fma(-(L[j * C + k] * d[k]), L[j * C + k], s);
    d[j] = s;
    ok = ok && s > 0.0f && s <= 3.402823466e+38f;
#pragma unroll
    for (int i = j + 1; i < C; i++)
    {
      float t = Qm[(S + i) * N + S + j];
#pragma unroll
      for (int k = 0; k < j; k++)
        t = det::fma(-(L[i * C + k] * d[k]), L[j * C + k], t);
      L[i * C + j] = t / s;
    }
  }
  return ok;
}

/** column j of Lk = -quu^-1 qux from the factors: x[a] = Lk(a, j) */
template <int S, int C>
MPPI_HD inline void gainColumn(const float* Qm, const float* L, const float* d, const int j, float* x)
{
  constexpr int N = S + C;
  float z[C];
#pragma unroll
  for (int a = 0; a < C; a++)
  {
    float s = -Qm[(S + a) * N + j];
#pragma unroll
    for (int k = 0; k < a; k++)
      s = det::fma(-L[a * C + k], z[k], s);
    z[a] = s;
  }
#pragma unroll
  for (int a = 0; a < C; a++)
    z[a] = z[a] / d[a];
#pragma unroll
  for (int a = C - 1; a >= 0; a--)
  {
    float s = z[a];
#pragma unroll
    for (int k = a + 1; k < C; k++)
      s = det::fma(-L[k * C + a], x[k], s);
    x[a] = s;
  }
}

/** entry (i, j) of the next Vxx, symmetrised; Lk[C][S] */
template <int S, int C>
MPPI_HD inline float vEntry(const float* Qm, const float* Lk, const int i, const int j)
{
  constexpr int N = S + C;
  float vij = Qm[i * N + j], vji = Qm[j * N + i];
#pragma unroll
  for (int a = 0; a < C; a++)
  {
    vij = det::fma(Qm[(S + a) * N + i], Lk[a * S + j], vij);
    vji = det::fma(Qm[(S + a) * N + j], Lk[a * S + i], vji);
  }
  return 0.5f * (vij + vji);
}

/** entry (i, j) of the boundary condition 0.5 (Qf + Qf^T) */
template <int S>
MPPI_HD inline float terminalEntry(const float* Qf, const int i, const int j)
{
  return 0.5f * (Qf[i * S + j] + Qf[j * S + i]);
}

/** the arrays of one step (the kernel keeps the same ones in LDS) */
template <int S, int C>
struct BackwardWork
{
  float V[S * S], F[S * (S + C)], W[S * (S + C)], Qm[(S + C) * (S + C)], Lk[C * S];
};

/**
 * The whole pass on the host (and the order the kernel's phases follow): A[T][S][S], B[T][S][C] continuous-time Jacobians
 * (Dynamics::computeGrad), Q[S][S], R[C][C], Qf[S][S] -> gains[T][S][C].
 * true: every row of gains written, *fail_step = -1.  false: step *fail_step failed; the rows above it (except T - 1) hold
 * their gains, that row, the rows below it and row T - 1 are untouched.
 */
template <int S, int C>
inline bool backwardPass(const float* A, const float* B, const float* Q, const float* R, const float* Qf, const float dt,
                         const int T, float* gains, int* fail_step)
{
  constexpr int N = S + C;
  BackwardWork<S, C> w;
  *fail_step = -1;
  for (int i = 0; i < S; i++)
    for (int j = 0; j < S; j++)
      w.V[i * S + j] = terminalEntry<S>(Qf, i, j);
  for (int i = 0; i < N * N; i++)
    w.Qm[i] = 0.0f;
  for (int k = T - 2; k >= 0; k--)
  {
    const float* Ak = A + (size_t)k * S * S;
    const float* Bk = B + (size_t)k * S * C;
    for (int i = 0; i < S; i++)
      for (int j = 0; j < N; j++)
        w.F[i * N + j] = fEntry<S, C>(Ak, Bk, dt, i, j);
    for (int i = 0; i < S; i++)
      for (int j = 0; j < N; j++)
        w.W[i * N + j] = wEntry<S, C>(w.V, w.F, i, j);
    for (int e = 0; e < S * S + C * N; e++)
    {
      int r, c;
      qIndex<S, C>(e, r, c);
      w.Qm[r * N + c] = qEntry<S, C>(w.F, w.W, costEntry<S, C>(Q, R, dt, r, c), r, c);
    }
    float L[C * C], d[C];
    if (!ldlt<S, C>(w.Qm, L, d))
    {
      *fail_step = k;
      return false;
    }
    for (int j = 0; j < S; j++)
    {
      float x[C];
      gainColumn<S, C>(w.Qm, L, d, j, x);
      for (int a = 0; a < C; a++)
      {
        w.Lk[a * S + j] = x[a];
        gains[((size_t)k * S + j) * C + a] = x[a];
      }
    }
    float Vn[S * S];
    for (int i = 0; i < S; i++)
      for (int j = 0; j < S; j++)
        Vn[i * S + j] = vEntry<S, C>(w.Qm, w.Lk, i, j);
    for (int i = 0; i < S * S; i++)
      w.V[i] = Vn[i];
  }
  if (T >= 1)
    for (int i = 0; i < S * C; i++)
      gains[(size_t)(T - 1) * S * C + i] = 0.0f;
  return true;
}

}  // namespace ddp
}  // namespace mppi

#endif
