/**
 * texture3d_host.hip — the HOST side of the shipped 3-D texture helper (include/mppi_amd/utils/texture_helpers/
 * three_d_texture_helper.hpp: the __host__ form of queryTexture and ThreeDTextureHelperHost) and the host form of the shipped
 * QuadrotorVolumeCost, for the tests.  TEST CODE ONLY.  Built two ways by tests/texture3d_oracle/__init__.py, host pass only:
 *   - as a library for ctypes (helper3d_* / volume_cost_* below);
 *   - with -DTEXTURE3D_HOST_MAIN as a stand-alone program whose main() walks the host class through the reference's
 *     UpdateTexture, UpdateTextureColumnMajor, UpdateTextureException and CopyDataToGPUSplitMiddle scenarios
 *     (tests/texture_helpers/three_d_texture_helper_test.cu) against a sink in host memory; that program is the one the address
 *     and undefined-behaviour sanitizers run on.
 * No HIP call is made by either.
 */
#include "mppi_amd/cost_functions/quadrotor/quadrotor_volume_cost.hpp"
#include "mppi_amd/model_params.h"
#include "mppi_amd/utils/texture_helpers/three_d_texture_helper.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static_assert(sizeof(mppi_quadrotor_volume_cost_params) == sizeof(QuadrotorVolumeCostParams), "POD block and plugin parameters differ");

namespace
{
using namespace mppi::texture;
using Host4 = ThreeDTextureHelperHost<1, 4>;

/** copyTo()'s sink in host memory: the "device" image and a log of (offset, floats) per write, allocations as (-1, floats) */
struct MemorySink
{
  std::vector<float> image;
  std::vector<std::pair<long long, long long>> log;
  const float* allocate(int, size_t floats)
  {
    image.assign(floats, -1.0f);
    log.emplace_back(-1, (long long)floats);
    return image.data();
  }
  bool write(int, size_t offset, const float* src, size_t floats)
  {
    log.emplace_back((long long)offset, (long long)floats);
    if (offset + floats > image.size())
      return false;
    memcpy(image.data() + offset, src, floats * sizeof(float));
    return true;
  }
};

/** a sink whose allocation fails, or whose writes fail from the second one on */
struct FailingSink : MemorySink
{
  bool fail_allocation = false;
  int writes_allowed = 1 << 30;
  const float* allocate(int index, size_t floats)
  {
    return fail_allocation ? nullptr : MemorySink::allocate(index, floats);
  }
  bool write(int index, size_t offset, const float* src, size_t floats)
  {
    return writes_allowed-- > 0 && MemorySink::write(index, offset, src, floats);
  }
};

template <int NC>
void fill(ThreeDTextureHelper<1, NC>& helper, const float* values, int width, int height, int depth, const int* modes,
          const float* border, const float* frame)
{
  TextureParams3D& t = helper.textures_[0];
  t.data = values;
  t.width = width;
  t.height = height;
  t.depth = depth;
  t.use = 1;
  for (int a = 0; a < 3; a++)
    t.address_mode[a] = modes[a];
  t.filter_mode = modes[3];
  memcpy(t.border_color, border, sizeof(t.border_color));
  memcpy(t.origin, frame, sizeof(t.origin));
  memcpy(t.rotations, frame + 3, sizeof(t.rotations));
  memcpy(t.resolution, frame + 12, sizeof(t.resolution));
}

template <int NC>
void query(const float* values, int width, int height, int depth, const int* modes, const float* border, const float* frame,
           const float* points, int n, int frame_kind, int batch, float* out)
{
  ThreeDTextureHelper<1, NC> helper;
  fill(helper, values, width, height, depth, modes, border, frame);
  if (batch)
  {
    for (int i = 0; i + batch <= n; i += batch)
    {
      const float(*w)[3] = reinterpret_cast<const float(*)[3]>(points + 3 * (size_t)i);
      if (batch == 1)
        helper.template queryTextureAtWorldPoseBatch<1>(0, w, out + (size_t)i * NC);
      else if (batch == 3)
        helper.template queryTextureAtWorldPoseBatch<3>(0, w, out + (size_t)i * NC);
      else
        helper.template queryTextureAtWorldPoseBatch<4>(0, w, out + (size_t)i * NC);
    }
    return;
  }
  for (int i = 0; i < n; i++)
  {
    const float* pt = points + 3 * (size_t)i;
    if (frame_kind == 0)
      helper.queryTexture(0, pt, out + (size_t)i * NC);
    else if (frame_kind == 1)
      helper.queryTextureAtMapPose(0, pt, out + (size_t)i * NC);
    else
      helper.queryTextureAtWorldPose(0, pt, out + (size_t)i * NC);
  }
}

Host4& host()
{
  static Host4 h;
  return h;
}
MemorySink& sink()
{
  static MemorySink s;
  return s;
}
QuadrotorVolumeCost& cost()
{
  static QuadrotorVolumeCost c;
  return c;
}
}  // namespace

extern "C" {
/** the shipped helper's host form; arguments as texture3d_oracle_query, batch = 0 / 1 / 3 / 4 */
void helper3d_query(const float* values, int width, int height, int depth, int channels, const int* modes, const float* border,
                    const float* frame, const float* points, int n, int frame_kind, int batch, float* out)
{
  if (channels == 4)
    query<4>(values, width, height, depth, modes, border, frame, points, n, frame_kind, batch, out);
  else
    query<1>(values, width, height, depth, modes, border, frame, points, n, frame_kind, batch, out);
}
float helper3d_wrap_z(float q, float period)
{
  return ThreeDTextureHelper<1, 1>::wrapZ(q, period);
}
/** 1 when the modes are refused (with the text in why), 0 when they can be sampled */
int helper3d_modes_refused(const int* address_mode, int depth, char* why, int n)
{
  const std::string s = addressModesRefusal(address_mode, depth);
  snprintf(why, (size_t)n, "%s", s.c_str());
  return !s.empty();
}

/* one ThreeDTextureHelperHost<1, 4> and one memory sink per process; every call returns 0, or -1 when the class threw */
int host3d_reset()
{
  host() = Host4();
  sink() = MemorySink();
  return 0;
}
int host3d_set_extent(int width, int height, int depth)
{
  try
  {
    return host().setExtent(0, width, height, depth) ? 1 : 0;
  }
  catch (const TextureUpdateError&)
  {
    return -1;
  }
}
int host3d_update_layer(int z, const float* values, int floats, int column_major)
{
  try
  {
    host().updateTexture(0, z, std::vector<float>(values, values + floats), column_major != 0);
    return 0;
  }
  catch (const TextureUpdateError&)
  {
    return -1;
  }
}
int host3d_update_volume(const float* values, int floats)
{
  try
  {
    host().updateTexture(0, std::vector<float>(values, values + floats));
    return 0;
  }
  catch (const TextureUpdateError&)
  {
    return -1;
  }
}
int host3d_set_address_mode(int axis, int mode)
{
  try
  {
    host().updateAddressMode(0, axis, mode);
    return 0;
  }
  catch (const TextureUpdateError&)
  {
    return -1;
  }
}
int host3d_values(float* out, int floats)
{
  const std::vector<float>& v = host().getCpuValues(0);
  if ((size_t)floats != v.size())
    return -1;
  memcpy(out, v.data(), v.size() * sizeof(float));
  return 0;
}
/** out[z] = 1 for a layer the next copy uploads; returns the depth */
int host3d_dirty(int* out, int n)
{
  const std::vector<bool>& d = host().getLayerCopy(0);
  for (int z = 0; z < n && z < (int)d.size(); z++)
    out[z] = d[(size_t)z];
  return (int)d.size();
}
/** copies into the memory sink; log[2 * i], log[2 * i + 1] = (offset, floats) of write i of THIS copy, (-1, floats) an allocation;
 *  returns the number of log entries */
int host3d_copy(long long* log, int max_entries)
{
  sink().log.clear();
  host().copyTo(sink());
  int n = 0;
  for (const auto& e : sink().log)
    if (n < max_entries)
    {
      log[2 * n] = e.first;
      log[2 * n + 1] = e.second;
      n++;
    }
  return n;
}
int host3d_image(float* out, int floats)
{
  if ((size_t)floats != sink().image.size())
    return -1;
  memcpy(out, sink().image.data(), sink().image.size() * sizeof(float));
  return 0;
}
/** the host object's parameters over the sink's image: what a kernel would see after the copy */
void host3d_query_image(const float* point, float* out4)
{
  Host4::Helper v = host().view();
  v.queryTexture(0, point, out4);
}

/* the shipped QuadrotorVolumeCost on the host */
void volume_cost_default_params(mppi_quadrotor_volume_cost_params* out)
{
  const QuadrotorVolumeCostParams d;
  memcpy(out, &d, sizeof(d));
}
void volume_cost_set_params(const mppi_quadrotor_volume_cost_params* block)
{
  memcpy((void*)&cost().params_, block, sizeof(*block));
}
/** values [depth][height][width] (kept by the caller); depth == 0: no volume */
void volume_cost_set_volume(const float* values, int depth, int height, int width, const float* frame)
{
  TextureParams3D& t = cost().volume_helper_.textures_[0];
  t.use = depth > 0 && height > 0 && width > 0;
  t.data = t.use ? values : nullptr;
  t.depth = depth;
  t.height = height;
  t.width = width;
  if (!t.use)
    return;
  memcpy(t.origin, frame, sizeof(t.origin));
  memcpy(t.rotations, frame + 3, sizeof(t.rotations));
  memcpy(t.resolution, frame + 12, sizeof(t.resolution));
}
float volume_cost_state_cost(const float* s)
{
  float y[13];
  memcpy(y, s, sizeof(y));
  return cost().computeStateCost(y, 0, nullptr, nullptr);
}
float volume_cost_terminal_cost(const float* s)
{
  float y[13];
  memcpy(y, s, sizeof(y));
  return cost().terminalCost(y);
}
void volume_cost_terms(const float* s, float* out)
{
  out[0] = cost().volumeValue(s);
  out[1] = cost().volumeCost(out[0]);
  out[2] = cost().quadraticCost(s);
}
int volume_cost_traits()
{
  const TextureParams3D& t = cost().volume_helper_.textures_[0];
  return (QuadrotorVolumeCost::MPPI_BARRIER_FREE_STEP ? 1 : 0) | (QuadrotorVolumeCost::MPPI_KERNARG_VIEWABLE ? 2 : 0) |
         ((t.address_mode[0] == ADDRESS_BORDER && t.address_mode[1] == ADDRESS_BORDER && t.address_mode[2] == ADDRESS_BORDER) ? 4 : 0);
}
}  // extern "C"

#ifdef TEXTURE3D_HOST_MAIN
#define CHECK(cond)                                                      \
  do                                                                     \
  {                                                                      \
    if (!(cond))                                                         \
    {                                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static std::vector<float> layerOf(float first, int texels)
{
  std::vector<float> v((size_t)texels * 4);
  for (int i = 0; i < texels; i++)
    for (int ch = 0; ch < 4; ch++)
      v[(size_t)i * 4 + ch] = first + (float)i + (float)ch;
  return v;
}

template <class F>
static bool throws(F f)
{
  try
  {
    f();
  }
  catch (const TextureUpdateError&)
  {
    return true;
  }
  return false;
}

int main()
{
  const int W = 10, H = 20;
  {  // UpdateTexture: two layers, row-major; texel i of the volume holds i, i + 1, i + 2, i + 3
    Host4 h;
    CHECK(h.setExtent(0, W, H, 2));
    CHECK(!h.setExtent(0, W, H, 2));
    h.updateTexture(0, 0, layerOf(0, W * H));
    h.updateTexture(0, 1, layerOf(200, W * H));
    const std::vector<float>& v = h.getCpuValues(0);
    CHECK(v.size() == (size_t)W * H * 2 * 4);
    for (int i = 0; i < W * H * 2; i++)
      for (int ch = 0; ch < 4; ch++)
        CHECK(v[(size_t)i * 4 + ch] == (float)(i + ch));
  }
  {  // UpdateTextureColumnMajor: three layers given column-major land row-major
    Host4 h;
    h.setExtent(0, W, H, 3);
    for (int k = 0; k < 3; k++)
      h.updateTexture(0, k, layerOf((float)(k * W * H), W * H), true);
    const std::vector<float>& v = h.getCpuValues(0);
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++)
          CHECK(v[((size_t)k * W * H + (size_t)i * W + j) * 4] == (float)(k * W * H + j * H + i));
  }
  {  // UpdateTextureException: a buffer of another texture's size, a layer outside the extent, bad extents, bad modes
    ThreeDTextureHelperHost<2, 4> h;
    h.setExtent(0, 10, 20, 1);
    h.setExtent(1, 30, 40, 1);
    CHECK(throws([&] { h.updateTexture(0, 0, layerOf(0, 30 * 40)); }));
    CHECK(throws([&] { h.updateTexture(0, 1, layerOf(0, 10 * 20)); }));
    CHECK(throws([&] { h.updateTexture(0, -1, layerOf(0, 10 * 20)); }));
    CHECK(throws([&] { h.updateTexture(0, std::vector<float>(7)); }));
    CHECK(throws([&] { h.setExtent(0, 10, 20, 0); }));
    CHECK(throws([&] { h.setExtent(2, 10, 20, 1); }));
    CHECK(throws([&] { h.updateAddressMode(0, 0, ADDRESS_WRAP); }));
    CHECK(throws([&] { h.updateAddressMode(0, 1, ADDRESS_WRAP); }));
    CHECK(throws([&] { h.updateAddressMode(0, 2, ADDRESS_WRAP); }));  // one layer: the period would be 0
    CHECK(throws([&] { h.updateAddressMode(0, 2, 7); }));
    h.updateAddressMode(0, 2, ADDRESS_BORDER);
    h.updateTexture(0, 0, layerOf(0, 10 * 20));
  }
  {  // CopyDataToGPUSplitMiddle: five layers, then the odd ones, then the even ones; only the changed layers travel
    Host4 h;
    MemorySink s;
    h.setExtent(0, W, H, 5);
    const size_t layer = (size_t)W * H * 4;
    for (int z = 0; z < 5; z++)
      h.updateTexture(0, z, layerOf((float)(z * W * H), W * H));
    for (int z = 1; z < 5; z += 2)
      h.updateTexture(0, z, layerOf((float)((z + 5) * W * H), W * H));
    CHECK(h.dirtySlices(0).size() == 1 && h.dirtySlices(0)[0] == std::make_pair(0, 5));
    CHECK(h.copyTo(s));
    CHECK(s.log.size() == 2 && s.log[0].first == -1 && s.log[1] == std::make_pair(0LL, (long long)(5 * layer)));
    for (bool d : h.getLayerCopy(0))
      CHECK(!d);
    CHECK(s.image == h.getCpuValues(0));
    const float expect1[6] = { 0, 600, 1200, 400, 1000, 1600 }, expect2[6] = { 2000, 1600, 1200, 2400, 2000, 1600 };
    const float zs[6] = { 0.1f, 0.2f, 0.3f, 0.5f, 0.6f, 0.7f };
    for (int i = 0; i < 6; i++)
    {
      const float pt[3] = { 0.0f, 0.0f, zs[i] };
      float out[4];
      h.view().queryTexture(0, pt, out);
      CHECK(fabsf(out[0] - expect1[i]) <= 4e-6f * fabsf(expect1[i]));
    }
    s.log.clear();
    for (int z = 0; z < 5; z += 2)
      h.updateTexture(0, z, layerOf((float)((z + 10) * W * H), W * H));
    const std::vector<std::pair<int, int>> runs = h.dirtySlices(0);
    CHECK(runs.size() == 3 && runs[0] == std::make_pair(0, 1) && runs[1] == std::make_pair(2, 1) && runs[2] == std::make_pair(4, 1));
    h.copyTo(s);
    CHECK(s.log.size() == 3);  // no new allocation, three one-layer slices
    for (int i = 0; i < 3; i++)
      CHECK(s.log[(size_t)i] == std::make_pair((long long)(2 * i * layer), (long long)layer));
    CHECK(s.image == h.getCpuValues(0));
    for (int i = 0; i < 6; i++)
    {
      const float pt[3] = { 0.0f, 0.0f, zs[i] };
      float out[4];
      h.view().queryTexture(0, pt, out);
      CHECK(fabsf(out[0] - expect2[i]) <= 4e-6f * fabsf(expect2[i]));
    }
    // two neighbouring layers are one slice; a copy with nothing changed writes nothing
    h.updateTexture(0, 1, layerOf(1, W * H));
    h.updateTexture(0, 2, layerOf(2, W * H));
    CHECK(h.dirtySlices(0).size() == 1 && h.dirtySlices(0)[0] == std::make_pair(1, 2));
    s.log.clear();
    h.copyTo(s);
    CHECK(s.log.size() == 1 && s.log[0] == std::make_pair((long long)layer, (long long)(2 * layer)));
    s.log.clear();
    h.copyTo(s);
    CHECK(s.log.empty());
    // a new extent: every layer again, into a new allocation
    CHECK(h.setExtent(0, W, H, 3));
    CHECK(h.dirtySlices(0).size() == 1 && h.dirtySlices(0)[0] == std::make_pair(0, 3));
    h.copyTo(s);
    CHECK(s.log.size() == 2 && s.log[0] == std::make_pair(-1LL, (long long)(3 * layer)) && s.image.size() == 3 * layer);
  }
  {  // a copy that fails leaves the host object knowing it: flags kept, texture not in use, the next copy does the work again
    Host4 h;
    FailingSink s;
    h.setExtent(0, W, H, 3);
    for (int z = 0; z < 3; z++)
      h.updateTexture(0, z, layerOf((float)(z * W * H), W * H));
    s.fail_allocation = true;
    CHECK(!h.copyTo(s));
    CHECK(h.dirtySlices(0).size() == 1 && h.dirtySlices(0)[0] == std::make_pair(0, 3));
    CHECK(!h.view().checkTextureUse(0) && h.view().textures_[0].data == nullptr);
    s.fail_allocation = false;
    CHECK(h.copyTo(s) && h.view().checkTextureUse(0) && h.dirtySlices(0).empty() && s.image == h.getCpuValues(0));
    h.updateTexture(0, 0, layerOf(7, W * H));
    h.updateTexture(0, 2, layerOf(9, W * H));
    s.writes_allowed = 1;  // the first slice goes through, the second does not
    CHECK(!h.copyTo(s));
    CHECK(h.dirtySlices(0).size() == 2);
    s.writes_allowed = 1 << 30;
    CHECK(h.copyTo(s) && h.dirtySlices(0).empty() && s.image == h.getCpuValues(0));
  }
  printf("texture3d host checks passed\n");
  return 0;
}
#endif
