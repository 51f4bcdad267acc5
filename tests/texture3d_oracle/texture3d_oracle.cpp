/**
 * texture3d_oracle.cpp — CPU restatement of the 3-D texture lookup and of QuadrotorVolumeCost for the tests
 * (tests/test_texture3d_helper.py, tests/test_quadrotor_volume.py).  TEST CODE ONLY.
 *
 * lookup(): the reference's fp32 HOST formula (utils/texture_helpers/three_d_texture_helper.cu:135-282) written the way the
 * reference walks it — one axis after the other with an early return of the border colour, the z wrap as two loops, the eight
 * corners by name — and NOT the way the shipped helper computes it (flags, selects, a closed-form wrap): the two are held to each
 * other bit for bit, and this one to the reference's own known answers (tests/texture_helpers/three_d_texture_helper_test.cu).
 * The transforms are the base class's (texture_helper.cu:94-124).  Where the shipped helper documents a difference from the
 * reference (a NaN coordinate, an axis of one texel) this file follows the helper; the tests do not go there.
 *
 * The cost: tests/quadrotor_oracle/quadrotor_oracle.cpp's quadratic cost (included as it stands) plus the volume terms, with the
 * plugin's order of additions (0 ulp against the kernels is the bar).  tests/texture3d_oracle/__init__.py compiles this file
 * TOGETHER with oracle/oracle_capi.cpp into one library, so the handle quadrotor_volume_oracle_create() returns is an
 * oracle::Controller of that library.
 */
#include "../quadrotor_oracle/quadrotor_oracle.cpp"

#include <cmath>
#include <vector>

namespace
{
enum
{
  CLAMP = 0,
  BORDER = 1,
  WRAP = 2
};

struct Volume
{
  const float* values = nullptr;  // [depth][height][width][channels]
  int width = 0, height = 0, depth = 0, channels = 1;
  int address[3] = { CLAMP, CLAMP, CLAMP };
  int point_filter = 0;
  float border[4] = { 0, 0, 0, 0 };
  float origin[3] = { 0, 0, 0 };
  float rot[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
  float resolution[3] = { 1, 1, 1 };

  float at(int x, int y, int z, int ch) const
  {
    return values[(((size_t)z * height + y) * width + x) * channels + ch];
  }
  void worldToMap(const float* world, float* in_map) const
  {
    const float off[3] = { world[0] - origin[0], world[1] - origin[1], world[2] - origin[2] };
    for (int r = 0; r < 3; r++)
      in_map[r] = rot[r][0] * off[0] + rot[r][1] * off[1] + rot[r][2] * off[2];
  }
  void mapToTex(const float* in_map, float* uvw) const
  {
    const int extent[3] = { width, height, depth };
    for (int a = 0; a < 3; a++)
    {
      uvw[a] = in_map[a] / resolution[a];
      uvw[a] /= (float)extent[a];
    }
  }
  /** returns false when the point is border on this axis */
  static bool addressAxis(float& q, int extent, int mode)
  {
    const float last = (float)(extent - 1);
    if (mode == BORDER)
      return !(q > last || q <= 0.0f);
    if (mode == WRAP)
    {
      while (q > last)
        q -= last;
      while (q < 0.0f)
        q += last;
      return true;
    }
    if (q > last)
      q = last;
    else if (q <= 0.0f)
      q = 0.0f;
    return true;
  }
  void lookup(const float* uvw, float* out) const
  {
    const int extent[3] = { width, height, depth };
    float q[3];
    for (int a = 0; a < 3; a++)
    {
      q[a] = uvw[a] * (float)extent[a];
      q[a] = q[a] - 0.5f;
      if (q[a] != q[a])
        q[a] = 0.0f;
    }
    for (int a = 0; a < 3; a++)
      if (!addressAxis(q[a], extent[a], address[a]))
      {
        for (int ch = 0; ch < channels; ch++)
          out[ch] = border[ch];
        return;
      }
    if (point_filter)
    {
      const int x = (int)std::round(q[0]), y = (int)std::round(q[1]), z = (int)std::round(q[2]);
      for (int ch = 0; ch < channels; ch++)
        out[ch] = at(x, y, z, ch);
      return;
    }
    int lo[3], hi[3];
    float d[3];
    for (int a = 0; a < 3; a++)
    {
      lo[a] = std::max(std::min((int)std::floor(q[a]), extent[a] - 2), 0);
      hi[a] = extent[a] > 1 ? lo[a] + 1 : lo[a];
      d[a] = extent[a] > 1 ? (q[a] - (float)lo[a]) / (float)(lo[a] + 1 - lo[a]) : 0.0f;
    }
    for (int ch = 0; ch < channels; ch++)
    {
      const float c000 = at(lo[0], lo[1], lo[2], ch), c100 = at(hi[0], lo[1], lo[2], ch);
      const float c010 = at(lo[0], hi[1], lo[2], ch), c001 = at(lo[0], lo[1], hi[2], ch);
      const float c110 = at(hi[0], hi[1], lo[2], ch), c101 = at(hi[0], lo[1], hi[2], ch);
      const float c011 = at(lo[0], hi[1], hi[2], ch), c111 = at(hi[0], hi[1], hi[2], ch);
      // along x to a square, along y to a line, along z to the point
      const float c00 = c000 * (1 - d[0]) + c100 * d[0];
      const float c01 = c001 * (1 - d[0]) + c101 * d[0];
      const float c10 = c010 * (1 - d[0]) + c110 * d[0];
      const float c11 = c011 * (1 - d[0]) + c111 * d[0];
      const float c0 = c00 * (1 - d[1]) + c10 * d[1];
      const float c1 = c01 * (1 - d[1]) + c11 * d[1];
      out[ch] = c0 * (1 - d[2]) + c1 * d[2];
    }
  }
};

struct QuadrotorVolumeCost : QuadrotorQuadraticCost
{
  float volume_coeff = 10.0f, crash_threshold = 0.9f, crash_coeff = 1000.0f;
  Volume volume;
  std::vector<float> volume_values;
  bool volume_in_use = false;

  QuadrotorVolumeCost()
  {
    for (int& mode : volume.address)
      mode = BORDER;
  }
  int setParams(const void* pod, size_t n) override
  {
    if (n != sizeof(mppi_quadrotor_volume_cost_params))
      return -1;
    const auto* block = static_cast<const mppi_quadrotor_volume_cost_params*>(pod);
    memcpy(&params_, pod, sizeof(params_));  // the quadratic block is the volume block's head
    volume_coeff = block->volume_coeff;
    crash_threshold = block->crash_threshold;
    crash_coeff = block->crash_coeff;
    return 0;
  }
  float valueAt(const float* s) const
  {
    if (!volume_in_use)
      return 0.0f;
    float in_map[3], uvw[3], v = 0.0f;
    volume.worldToMap(s, in_map);
    volume.mapToTex(in_map, uvw);
    volume.lookup(uvw, &v);
    return v;
  }
  float volumeTerm(float v) const
  {
    float total = volume_coeff * fmaxf(0.0f, v);
    if (v > crash_threshold)
      total += crash_coeff;
    return total;
  }
  float computeStateCost(const float* s, int t, int* crash) override
  {
    const float total = QuadrotorQuadraticCost::computeStateCost(s, t, crash) + volumeTerm(valueAt(s));
    return std::isnan(total) ? MAX_COST_VALUE : total;
  }
  float terminalCost(const float* s) override
  {
    const float cost = params_.terminal_cost_coeff * QuadrotorQuadraticCost::computeStateCost(s, 0, nullptr);
    return std::isnan(cost) ? MAX_COST_VALUE : cost;
  }
};

QuadrotorVolumeCost* volumeCost(void* h)
{
  return static_cast<QuadrotorVolumeCost*>(((oracle::Controller*)h)->cost.get());
}

void setFrame(Volume& v, const float* frame)
{
  for (int i = 0; i < 3; i++)
  {
    v.origin[i] = frame[i];
    v.resolution[i] = frame[12 + i];
    for (int j = 0; j < 3; j++)
      v.rot[i][j] = frame[3 + 3 * i + j];
  }
}
}  // namespace

static_assert(sizeof(mppi_quadrotor_volume_cost_params) == sizeof(mppi_quadrotor_cost_params) + 3 * sizeof(float), "block layout");

extern "C" {
/** modes: address_mode[3], filter; frame: origin[3], rotations[9] row-major, resolution[3]; frame_kind 0 texture coordinate,
 *  1 map pose, 2 world pose; points [n][3] -> out [n][channels] */
void texture3d_oracle_query(const float* values, int width, int height, int depth, int channels, const int* modes, const float* border,
                            const float* frame, const float* points, int n, int frame_kind, float* out)
{
  Volume v;
  v.values = values;
  v.width = width;
  v.height = height;
  v.depth = depth;
  v.channels = channels;
  for (int a = 0; a < 3; a++)
    v.address[a] = modes[a];
  v.point_filter = modes[3];
  for (int ch = 0; ch < 4; ch++)
    v.border[ch] = border[ch];
  setFrame(v, frame);
  for (int i = 0; i < n; i++)
  {
    float a[3] = { points[3 * i], points[3 * i + 1], points[3 * i + 2] }, b[3];
    if (frame_kind == 2)
    {
      v.worldToMap(a, b);
      std::copy(b, b + 3, a);
    }
    if (frame_kind >= 1)
    {
      v.mapToTex(a, b);
      std::copy(b, b + 3, a);
    }
    v.lookup(a, out + (size_t)i * channels);
  }
}

/** an oracle::Controller on QuadrotorDynamics + QuadrotorVolumeCost */
void* quadrotor_volume_oracle_create(int K, int T, int D, float dt, float lambda, float alpha, int num_iters)
{
  auto* c = new oracle::Controller();
  c->dyn.reset(new QuadrotorDynamics());
  c->cost.reset(new QuadrotorVolumeCost());
  c->dt = dt;
  c->lambda = lambda;
  c->alpha = alpha;
  c->num_iters = num_iters;
  c->init(K, T, D);
  return c;
}

/** values [depth][height][width]; frame as above; depth == 0 takes the volume away */
void quadrotor_volume_set_volume(void* h, const float* values, int depth, int height, int width, const float* frame)
{
  QuadrotorVolumeCost* c = volumeCost(h);
  c->volume_in_use = depth > 0 && height > 0 && width > 0;
  if (!c->volume_in_use)
    return;
  c->volume_values.assign(values, values + (size_t)depth * height * width);
  c->volume.values = c->volume_values.data();
  c->volume.depth = depth;
  c->volume.height = height;
  c->volume.width = width;
  setFrame(c->volume, frame);
}

/** out: the volume's value at the state's position, the volume term, the quadratic part */
void quadrotor_volume_terms(void* h, const float* s, float* out)
{
  QuadrotorVolumeCost* c = volumeCost(h);
  out[0] = c->valueAt(s);
  out[1] = c->volumeTerm(out[0]);
  out[2] = c->QuadrotorQuadraticCost::computeStateCost(s, 0, nullptr);
}

/** rolls the K rollouts of clamped controls v[K][T][4] out from x0 as oracle::rolloutCosts does; inside[k * T + t] = 1 when the
 *  output of step t lies inside the volume on every axis (0 < q <= extent - 1, the border rule) */
void quadrotor_volume_census(void* h, const float* x0, const float* v, int K, int T, int* inside)
{
  auto* ctl = (oracle::Controller*)h;
  QuadrotorVolumeCost* c = volumeCost(h);
  std::vector<float> x(13), xn(13), xdot(13), u(4), y(13), theta(1);
  for (int k = 0; k < K; k++)
  {
    std::copy(x0, x0 + 13, x.begin());
    std::fill(xdot.begin(), xdot.end(), 0.0f);
    for (int t = 0; t < T; t++)
    {
      std::copy(v + ((size_t)k * T + t) * 4, v + ((size_t)k * T + t) * 4 + 4, u.begin());
      ctl->dyn->enforceConstraints(x.data(), u.data());
      ctl->dyn->step(x.data(), xn.data(), xdot.data(), u.data(), y.data(), theta.data(), t, ctl->dt);
      float in_map[3], uvw[3];
      c->volume.worldToMap(y.data(), in_map);
      c->volume.mapToTex(in_map, uvw);
      const int extent[3] = { c->volume.width, c->volume.height, c->volume.depth };
      bool in = true;
      for (int a = 0; a < 3; a++)
      {
        const float q = uvw[a] * (float)extent[a] - 0.5f;
        in = in && !(q > (float)(extent[a] - 1) || q <= 0.0f);
      }
      inside[(size_t)k * T + t] = in;
      std::swap(x, xn);
    }
  }
}
}  // extern "C"
