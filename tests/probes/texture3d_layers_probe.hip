/**
 * texture3d_layers_probe.hip — ThreeDTextureHelperHost on the device: a 4 x 3 x 5 one-channel volume goes up whole, then layer 2
 * alone changes and copyToDevice() uploads that slice only.  Prints, before and after, the value at a point between layers 0 and 1
 * and at one between layers 2 and 3, the slices of the second copy, and whether the device allocation stayed where it was.
 * TEST CODE ONLY (tests/test_texture3d_helper.py).
 */
#include "mppi_amd/utils/texture_helpers/three_d_texture_helper.hpp"

#include <cstdio>
#include <vector>

using namespace mppi::texture;
using Host = ThreeDTextureHelperHost<1, 1>;

__global__ void queryKernel(Host::Helper helper, const float* __restrict__ points, int n, float* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    helper.queryTexture(0, points + 3 * i, out + i);
}

#define TRY(e)                                                                      \
  do                                                                                \
  {                                                                                 \
    const hipError_t err_ = (e);                                                    \
    if (err_ != hipSuccess)                                                         \
    {                                                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_));  \
      return 2;                                                                     \
    }                                                                               \
  } while (0)

int main()
{
  constexpr int W = 4, H = 3, D = 5, N = 2;
  Host host;
  DeviceTextureSink<1> sink;
  host.setExtent(0, W, H, D);
  std::vector<float> volume((size_t)W * H * D);
  for (size_t i = 0; i < volume.size(); i++)
    volume[i] = (float)i * 0.25f;
  host.updateTexture(0, volume);
  TRY(copyToDevice(host, sink));
  const float* first_allocation = sink.buffers[0];

  // tex coordinates: z * 5 - 0.5 = 0.4 (layers 0 and 1) and 2.6 (layers 2 and 3)
  const float points[N][3] = { { 0.4f, 0.6f, 0.18f }, { 0.4f, 0.6f, 0.62f } };
  mppi::engine::HipBuffer<float> d_points, d_out;
  TRY(d_points.alloc(3 * N));
  TRY(d_out.alloc(N));
  TRY(hipMemcpy(d_points, points, sizeof(points), hipMemcpyHostToDevice));
  float before[N], after[N];
  hipLaunchKernelGGL(queryKernel, dim3(1), dim3(64), 0, 0, host.view(), d_points, N, d_out);
  TRY(hipGetLastError());
  TRY(hipMemcpy(before, d_out, sizeof(before), hipMemcpyDeviceToHost));

  std::vector<float> layer((size_t)W * H);
  for (size_t i = 0; i < layer.size(); i++)
    layer[i] = 100.0f + (float)i;
  host.updateTexture(0, 2, layer);
  const auto slices = host.dirtySlices(0);
  TRY(copyToDevice(host, sink));
  hipLaunchKernelGGL(queryKernel, dim3(1), dim3(64), 0, 0, host.view(), d_points, N, d_out);
  TRY(hipGetLastError());
  TRY(hipMemcpy(after, d_out, sizeof(after), hipMemcpyDeviceToHost));

  float host_after[N];
  for (int i = 0; i < N; i++)
    host.hostView().queryTexture(0, points[i], &host_after[i]);
  printf("slices %zu first %d count %d\n", slices.size(), slices.empty() ? -1 : slices[0].first, slices.empty() ? -1 : slices[0].second);
  printf("same allocation %d\n", (int)(first_allocation == (const float*)sink.buffers[0]));
  for (int i = 0; i < N; i++)
    printf("point %d before %.9g after %.9g host %.9g\n", i, before[i], after[i], host_after[i]);
  return 0;
}
