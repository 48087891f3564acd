// Window maintenance of streaming inference (nb_asr_amd/streaming.py): every stage of a StreamingSession keeps the input frames it
// still needs (its left context) in a pitched window; a push moves them to the front of the stage's other window and appends the
// frames the producing stage has just made final behind them, in ONE pass per stage (ping-pong windows: source and destination never
// alias).  The pitch columns behind the new end are re-zeroed: the dense convolution fetches aligned 4-frame quads, and a shorter
// window than the last one would otherwise leave stale frames there that leak into its outputs.
//
// A wave per row (batch * channels rows of a few hundred frames): plain loads and stores, one atomic per wave for the optional
// per-utterance max|x| (the range bound of the f16x2 dense convolution, over the whole window).
#include "common.h"

namespace nbasr {

__global__ __launch_bounds__(256) void stream_window_kernel(
    const float* __restrict__ hist, int hist_ld, int hist_off, int n_hist, const float* __restrict__ src, int src_ld, int src_off, int n_new,
    float* __restrict__ dst, int dst_ld, int rows, int channels, unsigned* __restrict__ absmax)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                              // (wave-uniform)
    const float* const h = hist ? hist + static_cast<size_t>(r) * hist_ld + hist_off : nullptr;
    const float* const s = src ? src + static_cast<size_t>(r) * src_ld + src_off : nullptr;
    float* const d = dst + static_cast<size_t>(r) * dst_ld;
    const int n = n_hist + n_new;
    float m = 0.f;
    for (int j = lane; j < dst_ld; j += 64) {
        float v = 0.f;
        if (j < n_hist) v = h[j];
        else if (j < n) v = s[j - n_hist];
        d[j] = v;
        m = fmaxf(m, finite_abs(v));
    }
    if (absmax) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0 && m > 0.f) atomicMax(absmax + r / channels, __float_as_uint(m));      // (non-negative floats order as their bits)
    }
}

}  // namespace nbasr

using namespace nbasr;

extern "C" int nbasr_stream_window(const float* hist, int hist_ld, int hist_off, int n_hist, const float* src, int src_ld, int src_off, int n_new,
                                   float* dst, int dst_ld, int batch, int channels, float* absmax, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && channels > 0 && n_hist >= 0 && n_new >= 0 && hist_off >= 0 && src_off >= 0, NBASR_EINVAL,
                  "nbasr_stream_window: bad sizes (batch=%d channels=%d n_hist=%d n_new=%d hist_off=%d src_off=%d)",
                  batch, channels, n_hist, n_new, hist_off, src_off);
    NBASR_REQUIRE(n_hist == 0 || hist_off + n_hist <= hist_ld, NBASR_EINVAL,
                  "nbasr_stream_window: hist_off=%d + n_hist=%d exceeds hist_ld=%d", hist_off, n_hist, hist_ld);
    NBASR_REQUIRE(n_new == 0 || src_off + n_new <= src_ld, NBASR_EINVAL,
                  "nbasr_stream_window: src_off=%d + n_new=%d exceeds src_ld=%d", src_off, n_new, src_ld);
    NBASR_REQUIRE(n_hist + n_new <= dst_ld, NBASR_EINVAL, "nbasr_stream_window: %d frames do not fit dst_ld=%d", n_hist + n_new, dst_ld);
    const long long rows = static_cast<long long>(batch) * channels;
    NBASR_REQUIRE(rows <= (1ll << 30), NBASR_EINVAL, "nbasr_stream_window: %lld rows", rows);
    if (rows == 0 || dst_ld == 0) return NBASR_OK;
    NBASR_REQUIRE(dst && (n_hist == 0 || hist) && (n_new == 0 || src), NBASR_ENULL, "nbasr_stream_window: NULL pointer");
    NBASR_REQUIRE(n_hist == 0 || hist != dst, NBASR_EINVAL, "nbasr_stream_window: hist and dst must be different windows");
    if (absmax) zero_async(absmax, sizeof(float) * batch, as_stream(stream));
    hipLaunchKernelGGL(stream_window_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, as_stream(stream),
                       n_hist ? hist : nullptr, hist_ld, hist_off, n_hist, n_new ? src : nullptr, src_ld, src_off, n_new, dst, dst_ld,
                       static_cast<int>(rows), channels, reinterpret_cast<unsigned*>(absmax));
    return launch_status("nbasr_stream_window");
}
