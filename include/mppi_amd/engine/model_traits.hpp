/**
 * model_traits.hpp — detection of the optional members of plugin classes: what ModelT (model_instance.hpp) asks of a Dynamics or
 * Cost class before it offers a blob, a kernel form or a host method for it.
 */
#ifndef MPPI_AMD_MODEL_TRAITS_HPP_
#define MPPI_AMD_MODEL_TRAITS_HPP_

#include <type_traits>
#include <utility>

namespace mppi
{
namespace engine
{
template <class T, class = void>
struct has_fnn_helper : std::false_type
{
};
template <class T>
struct has_fnn_helper<T, std::void_t<decltype(std::declval<T&>().helper_.theta_d_)>> : std::true_type
{
};
template <class T, class = void>
struct has_grad_weights : std::false_type
{
};
/** dynamics whose computeGrad reads a parameter blob in device memory: `const float* gradWeights() const` */
template <class T>
struct has_grad_weights<T, std::void_t<decltype(std::declval<const T&>().gradWeights())>> : std::true_type
{
};
template <class T, class = void>
struct has_lstm_helper : std::false_type
{
};
template <class T>
struct has_lstm_helper<T, std::void_t<decltype(std::declval<T&>().lstm_.weights_d_)>> : std::true_type
{
};
template <class T, class = void>
struct has_host_leash : std::false_type
{
};
template <class T>
struct has_host_leash<T, std::void_t<decltype(std::declval<const T&>().enforceLeash((const float*)nullptr, (const float*)nullptr,
                                                                                     (const float*)nullptr, (float*)nullptr))>>
  : std::true_type
{
};
template <class T, class = void>
struct has_lstm_structure : std::false_type
{
};
/** dynamics whose LSTM shape can be changed at run time (setLSTMStructure, the "lstm_structure" blob) */
template <class T>
struct has_lstm_structure<T, std::void_t<decltype(std::declval<T&>().setLSTMStructure((const int*)nullptr, 0))>> : std::true_type
{
};
/** a replicated-lane form that names a sibling made for ONE rollout per wave (`using FINALIZE_FORM = ...`) */
template <class T, class = void>
struct has_finalize_form : std::false_type
{
};
template <class T>
struct has_finalize_form<T, std::void_t<typename T::FINALIZE_FORM>> : std::true_type
{
};
template <class T, class = void>
struct has_register_form : std::false_type
{
};
/** dynamics whose replicated-lane (FAST) variant exists for one network shape only (`register_form_`) */
template <class T>
struct has_register_form<T, std::void_t<decltype(std::declval<T&>().register_form_)>> : std::true_type
{
};
template <class T, class = void>
struct has_elevation_map : std::false_type
{
};
/** dynamics with a TwoDTextureHelper member `tex_helper_` (the elevation-map RACER models) */
template <class T>
struct has_elevation_map<T, std::void_t<decltype(std::declval<T&>().tex_helper_.textures_[0].data)>> : std::true_type
{
};
template <class T, class = void>
struct has_mean_unc_networks : std::false_type
{
};
/** dynamics with the mean and uncertainty LSTMs of RacerDubinsElevationLSTMUncertainty next to the steering one */
template <class T>
struct has_mean_unc_networks<T, std::void_t<decltype(std::declval<T&>().mean_lstm_d_), decltype(std::declval<T&>().unc_lstm_d_)>>
  : std::true_type
{
};
template <class T, class = void>
struct has_normals_map : std::false_type
{
};
/** dynamics with a second, four-channel map `normals_tex_helper_` (the suspension RACER models) */
template <class T>
struct has_normals_map<T, std::void_t<decltype(std::declval<T&>().normals_tex_helper_.textures_[0].data)>> : std::true_type
{
};
template <class T, class = void>
struct has_costmap : std::false_type
{
};
template <class T>
struct has_costmap<T, std::void_t<decltype(std::declval<T&>().costmap_d_)>> : std::true_type
{
};
/** channels of a has_costmap cost's map: `static constexpr int COSTMAP_CHANNELS = 4;` in the class (ARRobustCost: interleaved
 *  float[height][width][4] texels); absent: 1, a plain float[height][width] (ARStandardCost) */
template <class T, class = void>
struct costmap_channels : std::integral_constant<int, 1>
{
};
template <class T>
struct costmap_channels<T, std::void_t<decltype(T::COSTMAP_CHANNELS)>> : std::integral_constant<int, T::COSTMAP_CHANNELS>
{
};
template <class T, class = void>
struct has_cost_texture : std::false_type
{
};
/** a cost with a TwoDTextureHelper member `tex_helper_` (QuadrotorMapCost: the track map); ARStandardCost's costmap_d_ / r_c1
 *  form is has_costmap, and a class is one or the other (static_assert in ModelT) */
template <class T>
struct has_cost_texture<T, std::void_t<decltype(std::declval<T&>().tex_helper_.textures_[0].data)>> : std::true_type
{
};
template <class T, class = void>
struct has_cost_volume : std::false_type
{
};
/** a cost with a ThreeDTextureHelper member `volume_helper_` (QuadrotorVolumeCost: the clearance volume) */
template <class T>
struct has_cost_volume<T, std::void_t<decltype(std::declval<T&>().volume_helper_.textures_[0].depth)>> : std::true_type
{
};

}  // namespace engine
}  // namespace mppi

#endif
