"""The float64 restatements the kernel-form tests hold the engine to, in numpy alone: they share no code with the engine or
with the oracle (which mirrors det_math.h and the engine's reduction order, so it cannot see a bug both share).  Each
function names the reference lines it restates and derives its own rounding bound; the CPU tests of these functions are in
tests/test_kernel_sequence.py and tests/test_sampler_options_matrix.py."""
import numpy as np

SOFTMIN_RTOL = 2e-6
EPS32 = float(np.finfo(np.float32).eps)  # 2^-23


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_equal(a, b, nan_equal=False):
    """bit for bit; nan_equal: NaN equal to NaN (some RACER outputs are NaN at t = 0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    same = a.view(np.uint32) == b.view(np.uint32)
    if nan_equal:
        same |= np.isnan(a) & np.isnan(b)
    return bool(np.all(same))


def stats_of(stats, sysname):
    s = getattr(stats, sysname)
    return dict(baseline=s.baseline, normalizer=s.normalizer, free_energy_mean=s.free_energy_mean,
                free_energy_variance=s.free_energy_variance, free_energy_modified_variance=s.free_energy_modified_variance)


def softmin64(costs, v, lambda_):
    """u* = sum_k w_k v_k / sum_k w_k, w_k = exp(-(c_k - min c) / lambda), in float64"""
    c = np.asarray(costs, np.float64)
    w = np.exp(-(c - c.min()) / lambda_)
    return (w[:, None, None] * np.asarray(v, np.float64)).sum(0) / w.sum()


def stats64(costs, lambda_):
    """core/mppi_common.cu:1065-1081 evaluated in float64 on fp32 costs -> (values, bounds), both dicts with the keys
    baseline, normalizer, free_energy_mean, free_energy_variance, free_energy_modified_variance.

    The bounds are first-order fp32 rounding bounds, computed from K, u = 2^-24 and the costs themselves.  Weight k has the
    argument x_k = (c_k - b) / lambda; the engine forms it as fl(fl(c_k - b) * fl(1 / lambda)) (3 roundings: relative 3u,
    so 3u x_k absolute in the exponent) and det::exp adds <= 2 ulp = 4u, so w_k carries d_k = 3u x_k + 4u relative.  Any
    summation order of K positive terms adds at most (K - 1) u relative (Higham, Accuracy and Stability, 4.2), and the
    division by K one more u:
      e1 = sum w_k d_k / sum w_k + K u                       relative error of m  = mean w
      e2 = sum w_k^2 (2 d_k + u) / sum w_k^2 + K u           relative error of m2 = mean w^2 (one more rounding: the square)
    and then
      baseline   = min c                exact (a minimum of fp32 values is one of them)
      normalizer = K m                  2e-6 relative (the reference accumulates in double: only the weights round, e1 - K u)
      fe  = -lambda log m + b           lambda e1 + 8u (lambda |log m| + |b|): m's relative error becomes an absolute one
                                        through the log; log (2 ulp), the product and the sum round
      var = lambda (m2 - m^2)           lambda (e2 m2 + (2 e1 + u) m^2) + 3u |var|: m2 and m^2 carry their own relative
                                        errors and cancel, so the bound is relative to the operands, not to the difference
      mod = lambda (q + q^2 / 2), q = var / (m sqrt K)
                                        lambda (1 + |q|) dq + 4u |mod|, dq = d_var / (m sqrt K) + |q| (e1 + 6u)
    """
    c = np.asarray(costs, np.float32).astype(np.float64)
    K = c.size
    u = EPS32 / 2
    b = c.min()
    x = (c - b) / lambda_
    w = np.exp(-x)
    d = 3 * u * x + 4 * u
    e1 = (w * d).sum() / w.sum() + K * u
    e2 = (w * w * (2 * d + u)).sum() / (w * w).sum() + K * u
    mean, mean2 = w.mean(), (w * w).mean()
    fe = -lambda_ * np.log(mean) + b
    var = lambda_ * (mean2 - mean * mean)
    q = var / (mean * np.sqrt(K))
    mod = lambda_ * (q + 0.5 * q * q)
    d_fe = lambda_ * e1 + 8 * u * (lambda_ * abs(np.log(mean)) + abs(b))
    d_var = lambda_ * (e2 * mean2 + (2 * e1 + u) * mean * mean) + 3 * u * abs(var)
    d_q = d_var / (mean * np.sqrt(K)) + abs(q) * (e1 + 6 * u)
    d_mod = lambda_ * (1 + abs(q)) * d_q + 4 * u * abs(mod)
    vals = dict(baseline=b, normalizer=w.sum(), free_energy_mean=fe, free_energy_variance=var,
                free_energy_modified_variance=mod)
    bounds = dict(baseline=0.0, normalizer=SOFTMIN_RTOL * w.sum(), free_energy_mean=d_fe, free_energy_variance=d_var,
                  free_energy_modified_variance=d_mod)
    return vals, bounds


SG_TAPS = np.array([-3.0, 12.0, 17.0, 12.0, -3.0]) / 35.0


def smooth64(u, history):
    """controller.cuh:557-586: the 5-tap Savitzky-Golay filter over [hist0, hist1, u_0 .. u_{T-1}, u_{T-1}, u_{T-1}] ->
    (smoothed [T][C] in float64, bound [T][C]).  The engine filters in fp32 with the taps divided by 35 first: every tap, every
    product and each of the four additions rounds once, sum |tap_j| = 47/35 < 1.35, so the error is below
    (1 + 5 + 4) u 1.35 max|input| < 8 * 2^-23 * max|input| over the five inputs of the window (u = 2^-24)."""
    u = np.asarray(u, np.float64)
    T, C = u.shape
    buf = np.concatenate([np.asarray(history, np.float64).reshape(2, C), u, u[-1:], u[-1:]])
    out = np.zeros((T, C))
    peak = np.zeros((T, C))
    for j in range(5):
        out += SG_TAPS[j] * buf[j:j + T]
        peak = np.maximum(peak, np.abs(buf[j:j + T]))
    return out, 8 * EPS32 * peak


def slide64(u, steps, zero=None, scale=None):
    """controller.cuh:588-600 (the engine's default slide scale is 0: the tail is the zero control)"""
    u = np.asarray(u, np.float64)
    T, C = u.shape
    zero = np.zeros(C) if zero is None else np.asarray(zero, np.float64)
    scale = np.zeros(C) if scale is None else np.asarray(scale, np.float64)
    out = np.empty_like(u)
    for i in range(T):
        src = u[min(i + steps, T - 1)]
        out[i] = (src - zero) * scale + zero if i + steps > T - 1 else src
    return out


def save_history64(steps, u, history):
    """controller.cuh:602-615: history [2][C] (row 0 older) after a slide of `steps` of the control sequence u"""
    h = np.array(history, np.float64).reshape(2, -1)
    u = np.asarray(u, np.float64)
    if steps == 1:
        h = np.stack([h[1], u[0]])
    elif steps >= 2:
        h = np.stack([u[steps - 2], u[steps - 1]])
    return h


def constrain64(u, lo_hi, channels=None):
    """the base Dynamics::enforceConstraints with no deadband: a clamp of every (or only the listed) control channel"""
    u = np.array(u, np.float64)
    lo, hi = lo_hi
    ch = range(u.shape[1]) if channels is None else channels
    for c in ch:
        u[:, c] = np.minimum(np.maximum(u[:, c], lo[c]), hi[c])
    return u


def ranges(cfg, C):
    if cfg["ranges"] is None:
        return np.full(C, -np.inf), np.full(C, np.inf)
    r = np.asarray(cfg["ranges"], np.float64).reshape(C, 2)
    return r[:, 0], r[:, 1]


def ranges32(cfg, C):
    """the control ranges as the engine and the oracle hold them: rounded to fp32"""
    lo, hi = ranges(cfg, C)
    return lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)


def first_pure_rollout(K, pct):
    """the reference's compare (gaussian.cu:108): (float) k >= (1 - p) * (float) K in fp32 -> the first k that is pure noise"""
    edge = (np.float32(1.0) - np.float32(pct)) * np.float32(K)
    k = np.arange(K + 1)
    return int(k[k.astype(np.float32) >= edge][0])


def sample_rule64(mean, sigma, eps, stride, first_pure, lo_hi, decay, iteration=0):
    """setGaussianControls (gaussian.cu:99-127) and the base clamp in float64.  mean [T][C], sigma [T][C] undecayed, eps
    [K][T][C] -> (v [K][T][C], bound [K][T][C])"""
    m = np.asarray(mean, np.float64)[None]
    se = (decay ** iteration) * np.asarray(sigma, np.float64)[None] * np.asarray(eps, np.float64)
    K, T, _ = se.shape
    v = m + se
    pure = np.arange(K) >= first_pure
    v[pure] = se[pure]
    use_mean = np.zeros((K, T), bool)
    use_mean[0, :] = True
    use_mean[:, :stride] = True
    v[use_mean] = np.broadcast_to(m, v.shape)[use_mean]
    bound = 2.0 ** -21 * np.maximum(1.0, np.abs(m) + np.abs(se))
    lo, hi = lo_hi
    return np.minimum(np.maximum(v, lo), hi), bound


def likelihood_ratio64(v, mean, sigma, coeff, first_pure, lambda_, alpha):
    """(1/T) sum_t LR_t and (1/T) sum_t |LR_t| per rollout, LR_t = 0.5 lambda (1 - alpha) sum_j c_j mu_j (mu_j - 2 v_j) / sigma_j^2
    (gaussian.cu:480-569) with mu = 0 on pure-noise rollouts; v [K][T][C] clamped controls, mean / sigma [T][C]"""
    v = np.asarray(v, np.float64)
    K, T, _ = v.shape
    mu = np.broadcast_to(np.asarray(mean, np.float64)[None], v.shape).copy()
    mu[np.arange(K) >= first_pure] = 0.0
    s = np.asarray(sigma, np.float64)[None]
    lr = 0.5 * lambda_ * (1.0 - alpha) * (np.asarray(coeff, np.float64) * mu * (mu - 2.0 * v) / (s * s)).sum(2)
    return lr.sum(1) / T, np.abs(lr).sum(1) / T


def likelihood_ratio_bound(T, s_coeff, s_zero, lr_abs):
    return (T + 4) * EPS32 * (np.maximum(np.abs(s_coeff), np.abs(s_zero)) + lr_abs)
