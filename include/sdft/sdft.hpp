/*
 * sdft/sdft.hpp -- C++ facade `sdft::SDFT<T, F>` over the C-ABI of libsdft_hip.so.
 *
 * Mirrors the public interface of the reference's C++ header (cpp/src/sdft/sdft.h:29-255:
 * enum class Window :34-40, constructor :61, reset :97, size/window/latency :109-128,
 * sdft :135/:179/:193, isdft :205/:235/:249) so that code written against
 * `sdft::SDFT<float, double>` compiles unchanged; the work is done by the HIP kernels behind
 * the drop-in C functions of sdft/sdft.h.  `-I include/cpp` makes `#include <sdft/sdft.h>`
 * resolve to this facade for C++ hosts (the reference uses the same file name in its cpp tree).
 *
 * T (time domain) and F (frequency domain) may be float or double; long double has no GPU
 * representation and fails to compile.  std::complex<F> is layout-compatible with the C-ABI's
 * interleaved complex.  Pointers may be host or device pointers, as in the C API.
 */

#pragma once

#include <complex>
#include <cstddef>
#include <stdexcept>
#include <string>

extern "C" {
const char* sdft_hip_last_error(void);
#define SDFT_HPP_DECLARE(SUF, TD)                                                                   \
  void* sdft_hip_alloc_custom_##SUF(std::size_t dftsize, int window, double latency);               \
  void sdft_hip_free_##SUF(void* plan);                                                             \
  void sdft_hip_reset_##SUF(void* plan);                                                            \
  void sdft_hip_sdft_##SUF(void* plan, TD sample, void* dft);                                       \
  void sdft_hip_sdft_n_##SUF(void* plan, std::size_t n, const TD* samples, void* dfts);             \
  void sdft_hip_sdft_nd_##SUF(void* plan, std::size_t n, const TD* samples, void** dfts);           \
  TD sdft_hip_isdft_##SUF(void* plan, const void* dft);                                             \
  void sdft_hip_isdft_n_##SUF(void* plan, std::size_t n, const void* dfts, TD* samples);            \
  void sdft_hip_isdft_nd_##SUF(void* plan, std::size_t n, const void** dfts, TD* samples);            \
  long sdft_hip_sdft_every_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, void* dfts); \
  long sdft_hip_sdft_power_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first,     \
                                   std::size_t bin0, std::size_t nbins, void* power);                                    \
  long sdft_hip_sdft_power_sum_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                       std::size_t bin0, std::size_t nbins, void* sums);                               \
  long sdft_hip_sdft_power_peak_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                        std::size_t bin0, std::size_t nbins, int hold, void* peaks);                   \
  long sdft_hip_sdft_power_smooth_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                          std::size_t bin0, std::size_t nbins, double decay, void* state, void* smooth); \
  long sdft_hip_sdft_smooth_peak_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                         std::size_t bin0, std::size_t nbins, double decay, int hold, void* state, void* peaks); \
  long sdft_hip_sdft_power_moments_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                           std::size_t bin0, std::size_t nbins, void* moments);                        \
  int sdft_hip_set_filterbank_##SUF(void* plan, std::size_t nbands, const std::size_t* band_bin0, const std::size_t* band_nbins, \
                                    const void* weights);                                                               \
  std::size_t sdft_hip_filterbank_bands_##SUF(const void* plan);                                                       \
  long sdft_hip_sdft_filterbank_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, void* out); \
  long sdft_hip_sdft_band_peak_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, void* peaks); \
  int sdft_hip_set_pairs_##SUF(void* plan, std::size_t npairs, const std::size_t* pair_a, const std::size_t* pair_b);    \
  std::size_t sdft_hip_pairs_##SUF(const void* plan);                                                                  \
  long sdft_hip_sdft_cross_sum_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                       std::size_t bin0, std::size_t nbins, void* sums);                               \
  long sdft_hip_sdft_cross_smooth_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                          std::size_t bin0, std::size_t nbins, double decay, void* state, void* smooth); \
  long sdft_hip_sdft_lag_sum_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                     std::size_t bin0, std::size_t nbins, void* sums);                                 \
  int sdft_hip_set_array_##SUF(void* plan, std::size_t nch, const std::size_t* chan);                                  \
  std::size_t sdft_hip_array_channels_##SUF(const void* plan);                                                         \
  long sdft_hip_sdft_covariance_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first, \
                                        std::size_t bin0, std::size_t nbins, void* cov);                                \
  int sdft_hip_set_mix_##SUF(void* plan, std::size_t nout, std::size_t nch, const std::size_t* chan, const void* weights); \
  std::size_t sdft_hip_mix_outputs_##SUF(const void* plan);                                                            \
  long sdft_hip_sdft_mix_n_##SUF(void* plan, std::size_t n, const TD* samples, std::size_t every, std::size_t first,   \
                                 std::size_t bin0, std::size_t nbins, void* out);
SDFT_HPP_DECLARE(f32f64, float)
SDFT_HPP_DECLARE(f32f32, float)
SDFT_HPP_DECLARE(f64f64, double)
SDFT_HPP_DECLARE(f64f32, double)
#undef SDFT_HPP_DECLARE
}

namespace sdft
{
  /** Supported SDFT analysis window types (reference cpp/src/sdft/sdft.h:34-40). */
  enum class Window
  {
    Boxcar,
    Hann,
    Hamming,
    Blackman
  };

  /** The statistic of SDFT::power_peak(): the largest or the smallest power of a window (enum sdft_hip_hold). */
  enum class Hold
  {
    Max = 0,
    Min = 1
  };

  namespace detail
  {
    template <typename T, typename F> struct abi;   // undefined for unsupported type pairs
#define SDFT_HPP_ABI(SUF, TD, FD)                                                                   \
    template <> struct abi<TD, FD>                                                                  \
    {                                                                                               \
      static void* alloc(std::size_t n, int w, double l) { return sdft_hip_alloc_custom_##SUF(n, w, l); } \
      static void free(void* p) { sdft_hip_free_##SUF(p); }                                         \
      static void reset(void* p) { sdft_hip_reset_##SUF(p); }                                       \
      static void sdft(void* p, TD x, void* d) { sdft_hip_sdft_##SUF(p, x, d); }                    \
      static void sdft_n(void* p, std::size_t n, const TD* x, void* d) { sdft_hip_sdft_n_##SUF(p, n, x, d); } \
      static void sdft_nd(void* p, std::size_t n, const TD* x, void** d) { sdft_hip_sdft_nd_##SUF(p, n, x, d); } \
      static TD isdft(void* p, const void* d) { return sdft_hip_isdft_##SUF(p, d); }                \
      static void isdft_n(void* p, std::size_t n, const void* d, TD* y) { sdft_hip_isdft_n_##SUF(p, n, d, y); } \
      static void isdft_nd(void* p, std::size_t n, const void** d, TD* y) { sdft_hip_isdft_nd_##SUF(p, n, d, y); } \
      static long sdft_every_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, void* d) { return sdft_hip_sdft_every_n_##SUF(p, n, x, e, f, d); } \
      static long sdft_power_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_power_n_##SUF(p, n, x, e, f, b, k, d); } \
      static long sdft_power_sum_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_power_sum_n_##SUF(p, n, x, e, f, b, k, d); } \
      static long sdft_power_peak_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, int h, void* d) { return sdft_hip_sdft_power_peak_n_##SUF(p, n, x, e, f, b, k, h, d); } \
      static long sdft_power_smooth_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, double a, void* s, void* d) { return sdft_hip_sdft_power_smooth_n_##SUF(p, n, x, e, f, b, k, a, s, d); } \
      static long sdft_smooth_peak_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, double a, int h, void* s, void* d) { return sdft_hip_sdft_smooth_peak_n_##SUF(p, n, x, e, f, b, k, a, h, s, d); } \
      static long sdft_power_moments_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_power_moments_n_##SUF(p, n, x, e, f, b, k, d); } \
      static int set_filterbank(void* p, std::size_t nb, const std::size_t* b0, const std::size_t* bn, const void* w) { return sdft_hip_set_filterbank_##SUF(p, nb, b0, bn, w); } \
      static std::size_t filterbank_bands(const void* p) { return sdft_hip_filterbank_bands_##SUF(p); } \
      static long sdft_filterbank_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, void* d) { return sdft_hip_sdft_filterbank_n_##SUF(p, n, x, e, f, d); } \
      static long sdft_band_peak_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, void* d) { return sdft_hip_sdft_band_peak_n_##SUF(p, n, x, e, f, d); } \
      static int set_pairs(void* p, std::size_t np, const std::size_t* a, const std::size_t* b) { return sdft_hip_set_pairs_##SUF(p, np, a, b); } \
      static std::size_t pairs(const void* p) { return sdft_hip_pairs_##SUF(p); } \
      static long sdft_cross_sum_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_cross_sum_n_##SUF(p, n, x, e, f, b, k, d); } \
      static long sdft_cross_smooth_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, double a, void* s, void* d) { return sdft_hip_sdft_cross_smooth_n_##SUF(p, n, x, e, f, b, k, a, s, d); } \
      static long sdft_lag_sum_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_lag_sum_n_##SUF(p, n, x, e, f, b, k, d); } \
      static int set_array(void* p, std::size_t nc, const std::size_t* c) { return sdft_hip_set_array_##SUF(p, nc, c); } \
      static std::size_t array_channels(const void* p) { return sdft_hip_array_channels_##SUF(p); } \
      static long sdft_covariance_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_covariance_n_##SUF(p, n, x, e, f, b, k, d); } \
      static int set_mix(void* p, std::size_t no, std::size_t nc, const std::size_t* c, const void* w) { return sdft_hip_set_mix_##SUF(p, no, nc, c, w); } \
      static std::size_t mix_outputs(const void* p) { return sdft_hip_mix_outputs_##SUF(p); } \
      static long sdft_mix_n(void* p, std::size_t n, const TD* x, std::size_t e, std::size_t f, std::size_t b, std::size_t k, void* d) { return sdft_hip_sdft_mix_n_##SUF(p, n, x, e, f, b, k, d); } \
    };
    SDFT_HPP_ABI(f32f64, float, double)
    SDFT_HPP_ABI(f32f32, float, float)
    SDFT_HPP_ABI(f64f64, double, double)
    SDFT_HPP_ABI(f64f32, double, float)
#undef SDFT_HPP_ABI
  }

  /**
   * Sliding Discrete Fourier Transform (SDFT) on the GPU.
   * @tparam T Time domain data type: float (default) or double.
   * @tparam F Frequency domain data type: float or double (default and recommended).
   **/
  template <typename T = float, typename F = double>
  class SDFT
  {
    using api = detail::abi<T, F>;

  public:

    /** Creates a new SDFT plan (reference :61). Throws if the GPU cannot be set up. */
    SDFT(const std::size_t dftsize, const Window window = Window::Hann, const double latency = 1) :
      dftsize_(dftsize), window_(window), latency_(latency),
      plan_(api::alloc(dftsize, static_cast<int>(window), latency))
    {
      if (!plan_)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft::SDFT: ") + (e ? e : "plan allocation failed"));
      }
    }

    ~SDFT() { api::free(plan_); }

    SDFT(const SDFT&) = delete;
    SDFT& operator=(const SDFT&) = delete;
    SDFT(SDFT&& other) noexcept :
      dftsize_(other.dftsize_), window_(other.window_), latency_(other.latency_), plan_(other.plan_)
    {
      other.plan_ = nullptr;
    }

    /** Resets this SDFT plan instance to its initial state (reference :97). */
    void reset() { api::reset(plan_); }

    /** Returns the assigned number of DFT bins (reference :109). */
    std::size_t size() const { return dftsize_; }

    /** Returns the assigned analysis window type (reference :117). */
    Window window() const { return window_; }

    /** Returns the assigned synthesis latency factor (reference :125). */
    double latency() const { return latency_; }

    /** Estimates the DFT vector for the given sample (reference :135). */
    void sdft(const T sample, std::complex<F>* const dft) { api::sdft(plan_, sample, dft); }

    /** Estimates the DFT matrix (nsamples, dftsize) for the given sample array (reference :179). */
    void sdft(const std::size_t nsamples, const T* samples, std::complex<F>* const dfts)
    {
      api::sdft_n(plan_, nsamples, samples, dfts);
    }

    /** Same with an array of DFT row vectors (reference :193). */
    void sdft(const std::size_t nsamples, const T* samples, std::complex<F>** const dfts)
    {
      api::sdft_nd(plan_, nsamples, samples, reinterpret_cast<void**>(dfts));
    }

    /**
     * Decimated analysis (sdft_hip_sdft_every_n): the rows sdft() would write for the samples first, first + every, ...
     * < nsamples, dense in dfts; the plan's state advances over all samples.  Returns the number of rows written.
     * Streaming: the next call's first is first + rows * every - nsamples (rows > 0), else first - nsamples.
     **/
    std::size_t sdft_every(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                           std::complex<F>* const dfts)
    {
      const long rows = api::sdft_every_n(plan_, nsamples, samples, every, first, dfts);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_every_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Power-spectrogram analysis (sdft_hip_sdft_power_n): re*re + im*im of the bins bin0 <= k < bin0 + nbins of the rows
     * sdft() would write for the samples first, first + every, ... < nsamples, dense (rows, nbins) in out; the plan's state
     * advances over all samples and all bins.  Returns the number of rows written; streaming as with sdft_every().
     **/
    std::size_t power(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                      const std::size_t bin0, const std::size_t nbins, F* const out)
    {
      const long rows = api::sdft_power_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_power_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Pooled power analysis (sdft_hip_sdft_power_sum_n): the grid points first, first + every, ... cut the samples into windows;
     * row r of out, dense (rows, nbins), is the sum of power()'s every == 1 values over the r-th window for the bins
     * bin0 <= k < bin0 + nbins.  first > 0 makes row 0 the head window [0, first), which completes the previous call's last
     * row (add the two); the next call's first is sdft_every()'s.  Sums, not means: divide by the window's length for a mean.
     * The plan's state advances over all samples and all bins.  Returns the number of rows written.
     **/
    std::size_t power_sum(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                          const std::size_t bin0, const std::size_t nbins, F* const out)
    {
      const long rows = api::sdft_power_sum_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_power_sum_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Peak-hold analysis (sdft_hip_sdft_power_peak_n): power_sum()'s grid, windows, head row and layout; row r of out, dense
     * (rows, nbins), is the largest (Hold::Max) or the smallest (Hold::Min) of power()'s every == 1 values over the r-th window
     * for the bins bin0 <= k < bin0 + nbins, bit for bit one of them (NaN if the window holds a NaN).  first > 0 makes row 0 the
     * head window [0, first), which completes the previous call's last row (take the larger / smaller of the two); the next
     * call's first is sdft_every()'s.  The plan's state advances over all samples and all bins.  Returns the number of rows written.
     **/
    std::size_t power_peak(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                           const std::size_t bin0, const std::size_t nbins, const Hold hold, F* const out)
    {
      const long rows = api::sdft_power_peak_n(plan_, nsamples, samples, every, first, bin0, nbins, static_cast<int>(hold), out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_power_peak_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Smoothed power analysis (sdft_hip_sdft_power_smooth_n): the one-pole average s = a * s + (1 - a) * p of power()'s every == 1
     * values p, a = F(decay), advanced at every sample and kept on power()'s grid; out is dense (rows, nbins) [(channels, rows,
     * nbins)], row r the average after the sample first + r * every.  state is (nbins) [(channels, nbins)] numbers of the band,
     * host or device memory, read (s before the first sample) and written (s after the last); nullptr starts from zero and drops
     * the end value.  A stream passes state and sdft_every()'s next first from call to call.  decay is exp(-1 / tau) for a time
     * constant of tau samples and must round to 0 <= a < 1.  The plan's state advances over all samples and all bins.  Returns
     * the number of rows written.
     **/
    std::size_t power_smooth(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                             const std::size_t bin0, const std::size_t nbins, const double decay, F* const state, F* const out)
    {
      const long rows = api::sdft_power_smooth_n(plan_, nsamples, samples, every, first, bin0, nbins, decay, state, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_power_smooth_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n): power_peak()'s grid, windows, head row and layout with
     * power_smooth()'s sequence for the term: row r of out, dense (rows, nbins) [(channels, rows, nbins)], is the largest
     * (Hold::Max) or the smallest (Hold::Min) over the r-th window of s = a * s + (1 - a) * p, a = F(decay), advanced at every
     * sample and taken after the sample's update; s does not restart at a window.  state is (nbins) [(channels, nbins)] numbers
     * of the band, host or device memory, read (s before the first sample) and written (s after the last); nullptr starts from
     * zero and drops the end value.  A stream passes state and sdft_every()'s next first from call to call and, when first > 0,
     * takes the larger / smaller of row 0 and the previous call's last row.  Returns the number of rows written.
     **/
    std::size_t smooth_peak(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                            const std::size_t bin0, const std::size_t nbins, const double decay, const Hold hold, F* const state, F* const out)
    {
      const long rows = api::sdft_smooth_peak_n(plan_, nsamples, samples, every, first, bin0, nbins, decay, static_cast<int>(hold), state, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_smooth_peak_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Power-moments analysis (sdft_hip_sdft_power_moments_n): power_sum()'s grid, windows, head row and pointers; out is dense
     * (rows, nbins, 2) [(channels, rows, nbins, 2)]: per window and bin bin0 <= k < bin0 + nbins the pair (s1, s2), s1 the sum of
     * power()'s every == 1 values p over the window -- power_sum()'s value bit for bit -- and s2 the sum of fl(p * p).  Sums, not
     * means; first > 0 makes row 0 the head window [0, first), which completes the previous call's last row (add both
     * components); the next call's first is sdft_every()'s.  Consecutive sliding-DFT rows overlap in all but one sample, so a
     * detector built on the two sums is calibrated on the host's own noise.  The plan's state advances over all samples and all
     * bins.  Returns the number of rows written.
     **/
    std::size_t power_moments(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                              const std::size_t bin0, const std::size_t nbins, F* const out)
    {
      const long rows = api::sdft_power_moments_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_power_moments_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Installs (copies) a filterbank in the plan (sdft_hip_set_filterbank; host arrays): band b covers the bins
     * band_bin0[b] <= k < band_bin0[b] + band_nbins[b] with the weights weights[off_b + (k - band_bin0[b])], off_b the sum of the
     * band_nbins before it.  nbands == 0 removes it.
     **/
    void set_filterbank(const std::size_t nbands, const std::size_t* band_bin0, const std::size_t* band_nbins, const F* weights)
    {
      if (api::set_filterbank(plan_, nbands, band_bin0, band_nbins, weights) != 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_set_filterbank: ") + (e ? e : "failed"));
      }
    }
    /** Bands of the installed filterbank, 0 for none. */
    std::size_t filterbank_bands() const { return api::filterbank_bands(plan_); }

    /**
     * Filterbank analysis (sdft_hip_sdft_filterbank_n): per band of the installed filterbank the sum of weight * power over the
     * band's bins, for the rows power() would write for the samples first, first + every, ... < nsamples; out is dense
     * (rows, filterbank_bands()).  The plan's state advances over all samples and all bins.  Returns the number of rows written.
     **/
    std::size_t filterbank(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first, F* const out)
    {
      const long rows = api::sdft_filterbank_n(plan_, nsamples, samples, every, first, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_filterbank_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Band-peak analysis (sdft_hip_sdft_band_peak_n): per band of the installed filterbank the largest weight * power over the
     * band's bins and the bin that attains it, for the rows filterbank() would write; out is dense (rows, filterbank_bands(), 2):
     * [..][0] the value, [..][1] the absolute bin as an exactly representable integer of F.  Among the rounded products v of a
     * band in ascending bin order the pair is (v[i], i) with i the lowest bin of the largest value, or the lowest NaN bin if there
     * is one (numpy's argmax).  The plan's state advances over all samples and all bins.  Returns the number of rows written.
     **/
    std::size_t band_peak(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first, F* const out)
    {
      const long rows = api::sdft_band_peak_n(plan_, nsamples, samples, every, first, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_band_peak_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Installs (copies) a list of channel pairs in the plan (sdft_hip_set_pairs; host arrays): pair p is the channels
     * (pair_a[p], pair_b[p]); pairs may repeat and have a == b (the auto-spectrum).  npairs == 0 removes the list.
     **/
    void set_pairs(const std::size_t npairs, const std::size_t* pair_a, const std::size_t* pair_b)
    {
      if (api::set_pairs(plan_, npairs, pair_a, pair_b) != 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_set_pairs: ") + (e ? e : "failed"));
      }
    }
    /** Pairs of the installed list, 0 for none. */
    std::size_t pairs() const { return api::pairs(plan_); }

    /**
     * Pooled cross-spectrum analysis (sdft_hip_sdft_cross_sum_n): per pair (a, b) of the installed list the sum of
     * X_a conj(X_b) over the windows of power_sum()'s grid, for the bins bin0 <= k < bin0 + nbins; samples is
     * (channels, nsamples), out is dense (pairs(), rows, nbins).  Sums, not means; first > 0 makes row 0 the head window that
     * completes the previous call's last row.  The state of every channel advances over all samples and all bins.  Returns the
     * number of rows written.
     **/
    std::size_t cross_sum(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                          const std::size_t bin0, const std::size_t nbins, std::complex<F>* const out)
    {
      const long rows = api::sdft_cross_sum_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_cross_sum_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n): per pair (a, b) of the installed list the one-pole average
     * s = a * s + (1 - a) * X_a conj(X_b) of cross_sum()'s every == 1 term, each component on its own, a = F(decay), advanced at
     * every sample and kept on power()'s grid; samples is (channels, nsamples), out is dense (pairs(), rows, nbins), row r the
     * average after the sample first + r * every.  state is (pairs(), nbins) complex numbers of the band, read on entry and
     * written on return (nullptr: from zero, the end value is dropped); a stream passes it from call to call with the next first.
     * out may be nullptr when no row is kept.  The state of every channel advances over all samples and all bins.  Returns the
     * number of rows kept.
     **/
    std::size_t cross_smooth(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                             const std::size_t bin0, const std::size_t nbins, const double decay, std::complex<F>* const state,
                             std::complex<F>* const out)
    {
      const long rows = api::sdft_cross_smooth_n(plan_, nsamples, samples, every, first, bin0, nbins, decay, state, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_cross_smooth_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Lag-product analysis (sdft_hip_sdft_lag_sum_n): the sum of X[t] conj(X[t - 1]) over the windows of power_sum()'s grid, for
     * the bins bin0 <= k < bin0 + nbins; out is dense (rows, nbins) [(channels, rows, nbins)].  The angle of a sum over 2 pi,
     * times the sample rate, is the bin's power-weighted mean frequency over the window.  The row before the first sample is the
     * row of the plan's state (the zero row of a fresh plan).  Sums, not means; first > 0 makes row 0 the head window that
     * completes the previous call's last row.  The state advances over all samples and all bins.  Returns the number of rows
     * written.
     **/
    std::size_t lag_sum(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                        const std::size_t bin0, const std::size_t nbins, std::complex<F>* const out)
    {
      const long rows = api::sdft_lag_sum_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_lag_sum_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Installs (copies) an array in the plan (sdft_hip_set_array; a host list): an ordered list of nch distinct channels,
     * chan == nullptr for the channels 0 ... nch - 1.  nch == 0 removes the list.  Independent of set_pairs().
     **/
    void set_array(const std::size_t nch, const std::size_t* chan = nullptr)
    {
      if (api::set_array(plan_, nch, chan) != 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_set_array: ") + (e ? e : "failed"));
      }
    }
    /** Channels of the installed array, 0 for none. */
    std::size_t array_channels() const { return api::array_channels(plan_); }

    /**
     * Array covariance analysis (sdft_hip_sdft_covariance_n): cross_sum() for all pairs (i <= j) of the installed array; out is
     * dense (nch (nch + 1) / 2, rows, nbins), the upper triangle in row-major order, element i nch - i (i - 1) / 2 + (j - i)
     * the sums of X_chan[i] conj(X_chan[j]).  Every element has cross_sum()'s bits.  Returns the number of rows written.
     **/
    std::size_t covariance(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                           const std::size_t bin0, const std::size_t nbins, std::complex<F>* const out)
    {
      const long rows = api::sdft_covariance_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_covariance_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /**
     * Installs (copies) a mix in the plan (sdft_hip_set_mix; host memory): nout weight tables [nch][dftsize] for an ordered list
     * of nch distinct channels, chan == nullptr for the channels 0 ... nch - 1.  The weights are applied as written.  nout == 0
     * removes the mix.  Independent of set_pairs(), set_array() and the filterbank.
     **/
    void set_mix(const std::size_t nout, const std::size_t nch, const std::complex<F>* weights, const std::size_t* chan = nullptr)
    {
      if (api::set_mix(plan_, nout, nch, chan, weights) != 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_set_mix: ") + (e ? e : "failed"));
      }
    }
    /** Outputs of the installed mix, 0 for none. */
    std::size_t mix_outputs() const { return api::mix_outputs(plan_); }

    /**
     * Channel-mix analysis (sdft_hip_sdft_mix_n): the per-bin weighted sums of the installed mix at the rows of every()'s grid,
     * for the bins bin0 ... bin0 + nbins - 1; out is dense (nout, rows, nbins).  Returns the number of rows written.
     **/
    std::size_t mix(const std::size_t nsamples, const T* samples, const std::size_t every, const std::size_t first,
                    const std::size_t bin0, const std::size_t nbins, std::complex<F>* const out)
    {
      const long rows = api::sdft_mix_n(plan_, nsamples, samples, every, first, bin0, nbins, out);
      if (rows < 0)
      {
        const char* e = sdft_hip_last_error();
        throw std::runtime_error(std::string("sdft_hip_sdft_mix_n: ") + (e ? e : "failed"));
      }
      return static_cast<std::size_t>(rows);
    }

    /** Synthesizes a single sample from the given DFT vector (reference :205). */
    T isdft(const std::complex<F>* dft) { return api::isdft(plan_, dft); }

    /** Synthesizes the sample array from the given DFT matrix (reference :235). */
    void isdft(const std::size_t nsamples, const std::complex<F>* dfts, T* const samples)
    {
      api::isdft_n(plan_, nsamples, dfts, samples);
    }

    /** Same with an array of DFT row vectors (reference :249). */
    void isdft(const std::size_t nsamples, const std::complex<F>** dfts, T* const samples)
    {
      api::isdft_nd(plan_, nsamples, reinterpret_cast<const void**>(dfts), samples);
    }

    /** The underlying C-ABI plan (sdft_t*), for the additions declared in sdft/sdft_hip.h. */
    void* native_handle() const { return plan_; }

  private:

    std::size_t dftsize_;
    Window window_;
    double latency_;
    void* plan_;
  };
}
