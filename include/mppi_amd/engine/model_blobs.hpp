/**
 * model_blobs.hpp — what ModelT::setBlob and ModelT::setLSTMInitialState (model_instance.hpp) are written on: the count and dims
 * checks of a blob with their refusal texts, the upload into a buffer ModelT owns, and the binding of an uploaded map and its
 * frame to a TwoDTextureHelper or ThreeDTextureHelper texture entry.  The plugin classes keep plain non-owning pointers; nothing here owns memory.
 */
#ifndef MPPI_AMD_MODEL_BLOBS_HPP_
#define MPPI_AMD_MODEL_BLOBS_HPP_

#include <hip/hip_runtime.h>
#include <string>

#include "mppi_amd.h"
#include "hip_owned.hpp"

namespace mppi
{
namespace engine
{
/** "<name>: expected N floats, got M" unless count == expected */
inline bool expectCount(const std::string& name, size_t count, size_t expected, std::string& err)
{
  if (count == expected)
    return true;
  err = name + ": expected " + std::to_string(expected) + " floats, got " + std::to_string(count);
  return false;
}

/** a map's frame is origin[3], rotations[9] row-major, resolution[3] (updateOrigin / updateRotation / updateResolution,
 *  texture_helper.cu:192-268) */
constexpr size_t MAP_FRAME_FLOATS = 15;

inline bool expectFrameCount(const std::string& name, size_t count, std::string& err)
{
  if (count == MAP_FRAME_FLOATS)
    return true;
  err = name + ": expected 15 floats (origin[3], rotations[9], resolution[3])";
  return false;
}

/** a row-major map of `channels` floats per texel: dims {height, width}, or {height, width, channels} (interleaved texels) when
 *  there is more than one channel, with a product equal to count.
 *  spatial_rank == 3, a volume: dims {depth, height, width}, or {depth, height, width, channels}.  Refused, each with its own
 *  text: another rank; a channel count other than 1 or 4 (a texel is a float or a float4); a channel count other than the one
 *  the model reads; an extent of zero or less; a product other than count or beyond a 32-bit texel index. */
inline bool checkMapDims(const std::string& name, const int* dims, int ndims, size_t count, int channels, std::string& err,
                         int spatial_rank = 2)
{
  if (spatial_rank == 3)
  {
    if (ndims != 3 && ndims != 4)
    {
      err = name + ": dims must be {depth, height, width} or {depth, height, width, channels}, got rank " + std::to_string(ndims);
      return false;
    }
    const int given = ndims == 4 ? dims[3] : 1;
    if (given != 1 && given != 4)
    {
      err = name + ": a volume has 1 or 4 channels per texel, got " + std::to_string(given);
      return false;
    }
    if (given != channels)
    {
      err = name + ": this model reads " + std::to_string(channels) + " channel(s) per texel, got " + std::to_string(given);
      return false;
    }
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0)
    {
      err = name + ": every extent of {depth, height, width} must be positive";
      return false;
    }
    const unsigned long long texels = (unsigned long long)dims[0] * (unsigned long long)dims[1] * (unsigned long long)dims[2] * channels;
    if (texels != count || texels > 0x7fffffffULL)
    {
      err = name + ": depth*height*width*channels must equal count and fit a 32-bit index";
      return false;
    }
    return true;
  }
  const bool ok = ndims == (channels == 1 ? 2 : 3) && dims[0] > 0 && dims[1] > 0 && (channels == 1 || dims[2] == channels) &&
                  (size_t)dims[0] * dims[1] * channels == count;
  if (ok)
    return true;
  const std::string c = std::to_string(channels);
  err = channels == 1 ? name + ": dims must be {height, width} with height*width == count" :
                        name + ": dims must be {height, width, " + c + "} with height*width*" + c + " == count";
  return false;
}

/** frees the old blob, then uploads the new one */
inline mppi_status uploadBlob(HipBuffer<float>& dst, const float* src, size_t count, hipStream_t stream, std::string& err)
{
  hipError_t e = dst.alloc(count);
  if (e == hipSuccess)
    e = hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(stream);
  if (e != hipSuccess)
  {
    err = std::string("blob upload: ") + hipGetErrorString(e);
    return MPPI_ERR_HIP;
  }
  return MPPI_OK;
}

/** count floats into an uploaded blob at `offset` (the hidden / cell state behind an LSTM's parameters), in place; returns after
 *  the copy: the caller's buffer is pageable and may go away after the call */
inline mppi_status uploadTail(float* blob, size_t offset, const float* data, size_t count, const char* what, hipStream_t stream,
                              std::string& err)
{
  hipError_t e = hipMemcpyAsync(blob + offset, data, count * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(stream);
  if (e != hipSuccess)
  {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return MPPI_ERR_HIP;
  }
  return MPPI_OK;
}

/** TwoDTextureHelper::updateTexture + enableTexture (texture_helper.cu:135-190) for an entry whose map was uploaded into `buffer`
 *  with status st: the entry is in use only after a successful upload */
template <class TEX>
inline void bindMap(TEX& tex, const HipBuffer<float>& buffer, const int* dims, mppi_status st)
{
  tex.data = buffer;
  tex.height = dims[0];
  tex.width = dims[1];
  tex.use = (st == MPPI_OK);
}

/** bindMap for a volume entry (ThreeDTextureHelper): dims {depth, height, width, ...} */
template <class TEX>
inline void bindVolume(TEX& tex, const HipBuffer<float>& buffer, const int* dims, mppi_status st)
{
  tex.data = buffer;
  tex.depth = dims[0];
  tex.height = dims[1];
  tex.width = dims[2];
  tex.use = (st == MPPI_OK);
}

/** the MAP_FRAME_FLOATS of a frame into a texture entry */
template <class TEX>
inline void setMapFrame(TEX& tex, const float* data)
{
  for (int i = 0; i < 3; i++)
    tex.origin[i] = data[i];
  for (int i = 0; i < 9; i++)
    tex.rotations[i] = data[3 + i];
  for (int i = 0; i < 3; i++)
    tex.resolution[i] = data[12 + i];
}

}  // namespace engine
}  // namespace mppi

#endif
