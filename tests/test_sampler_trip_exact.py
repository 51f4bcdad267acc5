"""Round 9 on rolloutPipelineKernel: the sampler trip with fewer instructions computes what it computed before, bit for bit.

  CPU  the merge's quotient helper (engine/merge_wave.hpp: mergeDivisor / mergeQuotient(s)): its device arithmetic restated in
       fmaf as a stand-alone host program, seeded with the correctly rounded reciprocal and with that moved by +-1 ulp (what
       v_rcp_f32 is specified to), against `/` over 2^24 random pairs and the edges; outside the guard the helper is `/`
  GPU  the same pairs through mppi_det_eval id 15 (the single quotient and the packed quad), device against the host's `/`
  GPU  kernel forms: three iterations in one optimize() plus the flush, the streamed-merge form against the two-launch form
       bit for bit (u*, trajectory costs, statistics) and against the oracle (costs 0 ulp, u* within 1e-5), at the record
       counts at which the changed code takes another path and at horizons around the dynamics wave's 8-step and 4-step loops

The oracle check of a third iteration: with the fused reduction u* differs from the oracle's by rounding after every
iteration (tests/test_kernel_sequence.py), so the oracle is handed the mean the handle's third launch started from — u* of a
twin handle after two iterations, which is bit for bit the mean the sampler waves merge for themselves — and the third
generation of the Philox stream; its costs are then the handle's costs exactly, and its u* the handle's within 1e-5.
"""
import subprocess

import numpy as np
import pytest

import native_build as nb
from common import PHILOX_SEED, U_TOL, ulp_diff
from restate64 import bits


EXP_LO, EXP_HI = 127 - 60, 127 + 59   # merge_wave.hpp: MERGE_Q_EXP_LO / MERGE_Q_EXP_HI — the program checks them against the header
RANDOM_PAIRS = 1 << 24

QUOTIENT_PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mppi_amd/engine/merge_wave.hpp"

using mppi::kernels::mergeDivisorBenign;
using mppi::kernels::mergeQuotientBenign;

static uint32_t bits(float f)
{
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
/* the device branch of mergeDivisor + mergeQuotient(s), every operation one fmaf or one product; seed: the correctly rounded
 * reciprocal moved by `ulps` units in the last place */
static float core(float p, float q, int ulps)
{
  float r = 1.0f / q;
  if (ulps > 0)
    r = nextafterf(r, r > 0 ? INFINITY : -INFINITY);
  if (ulps < 0)
    r = nextafterf(r, 0.0f);
  r = fmaf(fmaf(-q, r, 1.0f), r, r);
  float y = p * r;
  y = fmaf(fmaf(-q, y, p), r, y);
  y = fmaf(fmaf(-q, y, p), r, y);
  return y;
}
int main(int argc, char** argv)
{
  if (argc < 4 || mppi::kernels::MERGE_Q_EXP_LO != (unsigned)atoi(argv[2]) || mppi::kernels::MERGE_Q_EXP_HI != (unsigned)atoi(argv[3]))
  {
    printf("usage: pairs.f32 EXP_LO EXP_HI (the header's guard: %u %u)\n", mppi::kernels::MERGE_Q_EXP_LO, mppi::kernels::MERGE_Q_EXP_HI);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return 2;
  std::vector<float> buf(1 << 16);
  unsigned long long n_fast = 0, n_slow = 0, n_bad = 0;
  size_t got;
  while ((got = fread(buf.data(), sizeof(float), buf.size(), f)) > 0)
    for (size_t i = 0; i + 1 < got; i += 2)
    {
      const float p = buf[i], q = buf[i + 1], want = p / q;
      // the helper: inside the guard the core, outside it the division itself (mergeQuotient's host build is `/` throughout,
      // so it is called too: the header's own host path must be the division)
      if (bits(mppi::kernels::mergeQuotient(p, mppi::kernels::mergeDivisor(q))) != bits(want))
        n_bad++;
      if (!(mergeDivisorBenign(q) && mergeQuotientBenign(p)))
      {
        n_slow++;
        continue;
      }
      n_fast++;
      for (int ulps = -1; ulps <= 1; ulps++)
      {
        const float y = core(p, q, ulps);
        if (bits(y) != bits(want) && n_bad++ < 10)
          printf("MISMATCH p=%a q=%a seed%+d: core %a (%08x), division %a (%08x)\n", p, q, ulps, y, bits(y), want, bits(want));
      }
    }
  fclose(f);
  printf("through the core %llu, through the division %llu, mismatches %llu\n", n_fast, n_slow, n_bad);
  return n_bad ? 1 : 0;
}
"""


def _f(u):
    return np.asarray(u, np.uint32).view(np.float32)


def _benign(x, divisor=False):
    """the guard of merge_wave.hpp restated: biased exponent in [EXP_LO, EXP_HI]; a divisor also not all ones in the significand"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    e = (b >> 23) & 0xff
    ok = (e >= EXP_LO) & (e <= EXP_HI)
    if divisor:
        ok &= (b & 0x7fffff) != 0x7fffff
    return ok


_PAIRS = None


def _pairs():
    """(p, q) float32 arrays: the edges (every eta with every tot) and RANDOM_PAIRS random pairs, built once"""
    global _PAIRS
    if _PAIRS is not None:
        return _PAIRS
    lo, hi = np.float32(2.0) ** (EXP_LO - 127), np.float32(2.0) ** (EXP_HI + 1 - 127)   # the guard admits [lo, hi)
    around = lambda v: [np.nextafter(np.float32(v), np.float32(0)), np.float32(v), np.nextafter(np.float32(v), np.float32(np.inf))]
    etas = [1.0, 16384.0, 3.0, 16383.0] + [2.0 ** e for e in range(-62, 63)] + around(lo) + around(hi)
    # significands of all ones (the divisor's own exception) and their neighbours, at both ends and in the middle of the range
    etas += list(_f([((e + 127) << 23) | mant for e in (-60, -1, 0, 1, 13, 59) for mant in (0x7fffff, 0x7ffffe, 0x7ffffd, 1)]))
    etas += [-1.0, 0.0, -0.0, np.inf, np.nan, _f(1)]   # divisors the guard refuses as well
    sub_min, sub_max = _f(1), _f(0x007fffff)
    tots = [0.0, -0.0, sub_min, sub_max, -sub_min, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 3.0, 1e-3, -7.25]
    for lim in (lo, hi):
        for v in around(lim):
            tots += [v, -v]
    etas, tots = np.array(etas, np.float32), np.array(tots, np.float32)
    pe, qe = np.repeat(tots, len(etas)), np.tile(etas, len(tots))
    rng = np.random.Generator(np.random.Philox(9))
    n = RANDOM_PAIRS // 2
    # half over the whole guarded range (random exponent and significand, either sign of p) ...
    expo = lambda: rng.integers(EXP_LO, EXP_HI + 1, n, dtype=np.uint32) << np.uint32(23)
    mant = lambda: rng.integers(0, 1 << 23, n, dtype=np.uint32)
    q1 = _f(expo() | mant())
    p1 = _f(expo() | mant() | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)))
    # ... half at the merge's own magnitudes: eta in [1, K], |tot| from 2^-8 to a few thousand
    q2 = rng.uniform(1.0, 16384.0, n).astype(np.float32)
    p2 = (rng.uniform(-1.0, 1.0, n) * 2.0 ** rng.integers(-8, 16, n)).astype(np.float32)
    _PAIRS = (np.concatenate([pe, p1, p2]), np.concatenate([qe, q1, q2]))
    return _PAIRS


def test_quotient_helper_arithmetic_equals_division_on_the_host(tmp_path):
    p, q = _pairs()
    assert p.size >= RANDOM_PAIRS + 1000
    src, exe, data = tmp_path / "quotient.hip", tmp_path / "quotient", tmp_path / "pairs.f32"
    src.write_text(QUOTIENT_PROGRAM)
    np.stack([p, q], axis=1).tofile(data)
    nb.build(exe, nb.hip_host(src), [src], "quotient")
    r = subprocess.run([str(exe), str(data), str(EXP_LO), str(EXP_HI)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    # the program's split of the pairs is the guard as this file states it: a pair outside the guard took `/`
    inside = int((_benign(p) & _benign(q, divisor=True)).sum())
    assert "through the core %d, through the division %d, mismatches 0" % (inside, p.size - inside) in r.stdout, r.stdout[-500:]
    assert inside >= RANDOM_PAIRS and p.size - inside >= 1000


@pytest.mark.gpu
def test_quotient_helper_on_the_device_equals_host_division(gpu):
    import mppi_generic_amd as m
    p, q = _pairs()
    x = np.stack([p, q], axis=1).reshape(-1)
    y = m.det_eval(15, x)
    k = np.arange(p.size)
    with np.errstate(all="ignore"):
        single = p / q
        quad = p[(k + (k & 3)) % p.size] / q     # entry k & 3 of the packed quad (p_k .. p_k+3) / q_k
    for name, got, want in (("mergeQuotient", y[0::2], single), ("mergeQuotients", y[1::2], quad)):
        bad = np.flatnonzero(bits(got) != bits(want))
        print("%s: %d of %d pairs differ from the host's division" % (name, bad.size, p.size))
        assert bad.size == 0, "%s: pair %d, p=%r q=%r: device %r, host %r" % (name, bad[0], p[bad[0]], q[bad[0]], got[bad[0]],
                                                                            want[bad[0]])


# ------------------------------------------------------------------ kernel forms ----------------------------------------
# (K, T): 256 records — the full-record path — with one / two / two / three 8-step trips of the dynamics wave;
# 255 records: the select path; 65: a partly filled second record slot; one record
STREAMED_KT = [(16384, 8), (16384, 16), (16384, 20), (16384, 28), (16320, 16), (4160, 24), (64, 12)]
# T * C is no multiple of 4 for either model: two launches per iteration; horizons with a tail behind the 4-step groups
PLAIN_KT = [(128, 7), (128, 9), (128, 15), (128, 17), (128, 23)]
MODELS = {"cartpole": "cartpole-vanilla-pipeline64x1x1", "di": "double_integrator-vanilla-pipeline64x1x1"}


def _stats(e):
    s = e.getStats().real_sys
    return np.array([s.baseline, s.normalizer, s.free_energy_mean, s.free_energy_variance, s.free_energy_modified_variance],
                    np.float32)


def _case(model):
    from kernel_forms import build_cases
    found = [c for c in build_cases() if c["id"] == MODELS[model]]
    assert found, "%s is not among the registered kernel forms" % MODELS[model]
    return found[0]


def _run(model, K, T, streamed):
    import pyoracle as po
    from kernel_forms import check_form, make_handles
    case = _case(model)
    tag = "%s K=%d T=%d" % (case["id"], K, T)
    cfg, a, orc, _ = make_handles(case, K, T)
    twin = make_handles(case, K, T)[1]                                    # the mean the third launch starts from
    handles = [a, twin]
    if streamed:
        handles.append(make_handles(case, K, T, env=dict(MPPI_AMD_NO_STREAM_MERGE="1"))[1])
    try:
        C = a.CONTROL_DIM
        assert ((T * C) % 4 == 0) == streamed, tag
        for e in handles:
            e.uploadState(cfg["x0"])
            e.setSeed(PHILOX_SEED)
        a.optimize(3)
        twin.optimize(2)
        check_form(case, a, tag, streamed=streamed)
        u3, costs3 = a.getOptimalControlSeq(), a.getSampledCostSeq()      # (the reads flush the pending records)
        assert np.isfinite(costs3).all() and np.isfinite(u3).all(), tag
        if streamed:
            b = handles[2]
            b.optimize(3)
            check_form(case, b, tag + " [two-launch]", streamed=False)
            assert np.array_equal(bits(u3), bits(b.getOptimalControlSeq())), tag + ": u* differs from the two-launch form"
            assert np.array_equal(bits(costs3), bits(b.getSampledCostSeq())), tag + ": costs differ from the two-launch form"
            assert np.array_equal(bits(_stats(a)), bits(_stats(b))), tag + ": statistics differ from the two-launch form"
        u_orc = orc.iterate(cfg["x0"], twin.getOptimalControlSeq(), po.philox_normal(PHILOX_SEED, 2, K, T, C), 1, 2)
        dc, du = int(ulp_diff(costs3, orc.costs()).max()), float(np.abs(u3 - u_orc).max())
        print("%s: costs %d ulp, u* %g from the oracle" % (tag, dc, du))
        assert dc == 0, "%s: trajectory costs differ from the oracle by up to %d ulp" % (tag, dc)
        assert du <= U_TOL, "%s: u* differs from the oracle by %g" % (tag, du)
    finally:
        for e in handles:
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("K,T", STREAMED_KT, ids=["%dx%d" % kt for kt in STREAMED_KT])
def test_streamed_sampler_trip_keeps_its_bits(gpu, model, K, T):
    _run(model, K, T, streamed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("K,T", PLAIN_KT, ids=["%dx%d" % kt for kt in PLAIN_KT])
def test_two_launch_form_at_ragged_horizons(gpu, model, K, T):
    _run(model, K, T, streamed=False)
