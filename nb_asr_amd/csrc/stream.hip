// Window maintenance of streaming inference (nb_asr_amd/streaming.py): every stage of a StreamingSession keeps the input frames it
// still needs (its left context) in a pitched window; a push moves them to the front of the stage's other window and appends the
// frames the producing stage has just made final behind them, in ONE pass per stage (ping-pong windows: source and destination never
// alias).  The pitch columns behind the new end are re-zeroed: the dense convolution fetches aligned 4-frame quads, and a shorter
// window than the last one would otherwise leave stale frames there that leak into its outputs.
//
// A wave per row (batch * channels rows of a few hundred frames): plain loads and stores, one atomic per wave for the optional
// per-utterance max|x| (the range bound of the f16x2 dense convolution, over the whole window).
//
// The bf16 windows of a bfloat16 session (nbasr_stream_window_bf16): the same wave per row, a lane per 16-byte chunk of the destination,
// so every store is one whole aligned chunk (rows are pitched to 8 frames).  The retained and the new frames start at arbitrary element
// offsets, so the lane GATHERS its 8 frames with element-sized loads (2 bytes from bf16 rows, 4 from the fp32 frames of a waveform
// session) -- chosen over aligned dword loads with a funnel shift because those read up to one element outside the named range and
// the rows are a few hundred frames: the launch, not the loads, is what a window costs.  An fp32 frame is rounded by pack_bf16x2, the
// rounding of every other bf16 store (nearest even, NaN stays NaN); bf16 frames are copied as bits.  No range bound: the bf16 path has
// no range pass.
#include "common.h"
#include "storage.h"

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

// one frame of the window as bfloat16 bits: retained (bits copied), new (bits copied or an fp32 frame rounded), or a pitch column (0)
template <bool SRC_F32> __device__ __forceinline__ unsigned window_frame_bf16(const unsigned short* __restrict__ h, const void* __restrict__ s,
                                                                              int j, int n_hist, int n)
{
    if (j < n_hist) return h[j];
    if (j >= n) return 0u;
    if constexpr (SRC_F32) return pack_bf16x2(static_cast<const float*>(s)[j - n_hist], 0.f) & 0xffffu;
    else return static_cast<const unsigned short*>(s)[j - n_hist];
}

template <bool SRC_F32> __global__ __launch_bounds__(256) void stream_window_bf16_kernel(
    const unsigned short* __restrict__ hist, int hist_ld, int hist_off, int n_hist, const void* __restrict__ src, int src_ld, int src_off,
    int n_new, unsigned short* __restrict__ dst, int dst_ld, int rows)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                              // (wave-uniform)
    const unsigned short* const h = hist ? hist + static_cast<size_t>(r) * hist_ld + hist_off : nullptr;
    const size_t s_at = static_cast<size_t>(r) * src_ld + src_off;
    const void* const s = !src ? nullptr : SRC_F32 ? static_cast<const void*>(static_cast<const float*>(src) + s_at)
                                                   : static_cast<const void*>(static_cast<const unsigned short*>(src) + s_at);
    u4v* const d = reinterpret_cast<u4v*>(dst + static_cast<size_t>(r) * dst_ld);       // (dst_ld % 8 == 0, dst 16-byte aligned)
    const int n = n_hist + n_new;
    for (int c = lane; c < dst_ld / 8; c += 64) {
        unsigned w[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int j = 8 * c + 2 * p;
            w[p] = window_frame_bf16<SRC_F32>(h, s, j, n_hist, n) | (window_frame_bf16<SRC_F32>(h, s, j + 1, n_hist, n) << 16);
        }
        d[c] = u4v{w[0], w[1], w[2], w[3]};
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

extern "C" int nbasr_stream_window_bf16(const void* hist, int hist_ld, int hist_off, int n_hist, const void* src, int src_dtype, int src_ld,
                                        int src_off, int n_new, void* dst, int dst_ld, int batch, int channels, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && channels > 0 && n_hist >= 0 && n_new >= 0 && hist_off >= 0 && src_off >= 0 && dst_ld >= 0, NBASR_EINVAL,
                  "nbasr_stream_window_bf16: bad sizes (batch=%d channels=%d n_hist=%d n_new=%d hist_off=%d src_off=%d dst_ld=%d)",
                  batch, channels, n_hist, n_new, hist_off, src_off, dst_ld);
    NBASR_REQUIRE(dst_ld % 8 == 0, NBASR_EALIGN, "nbasr_stream_window_bf16: dst_ld=%d is not a multiple of 8 (bf16 rows are whole 16-byte chunks)", dst_ld);
    NBASR_REQUIRE(src_dtype == NBASR_F32 || src_dtype == NBASR_BF16, NBASR_EINVAL,
                  "nbasr_stream_window_bf16: src_dtype=%d is neither NBASR_F32 nor NBASR_BF16", src_dtype);
    NBASR_REQUIRE(n_hist == 0 || static_cast<long long>(hist_off) + n_hist <= hist_ld, NBASR_EINVAL,
                  "nbasr_stream_window_bf16: hist_off=%d + n_hist=%d exceeds hist_ld=%d", hist_off, n_hist, hist_ld);
    NBASR_REQUIRE(n_new == 0 || static_cast<long long>(src_off) + n_new <= src_ld, NBASR_EINVAL,
                  "nbasr_stream_window_bf16: src_off=%d + n_new=%d exceeds src_ld=%d", src_off, n_new, src_ld);
    NBASR_REQUIRE(static_cast<long long>(n_hist) + n_new <= dst_ld, NBASR_EINVAL, "nbasr_stream_window_bf16: %lld frames do not fit dst_ld=%d",
                  static_cast<long long>(n_hist) + n_new, dst_ld);
    const long long rows = static_cast<long long>(batch) * channels;
    NBASR_REQUIRE(rows <= (1ll << 30), NBASR_EINVAL, "nbasr_stream_window_bf16: %lld rows", rows);
    if (rows == 0 || dst_ld == 0) return NBASR_OK;
    NBASR_REQUIRE(dst && (n_hist == 0 || hist) && (n_new == 0 || src), NBASR_ENULL, "nbasr_stream_window_bf16: NULL pointer");
    NBASR_REQUIRE(aligned16(dst), NBASR_EALIGN, "nbasr_stream_window_bf16: dst is not 16-byte aligned");
    NBASR_REQUIRE(n_hist == 0 || hist != dst, NBASR_EINVAL, "nbasr_stream_window_bf16: hist and dst must be different windows");
    const auto kernel = src_dtype == NBASR_F32 ? stream_window_bf16_kernel<true> : stream_window_bf16_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, as_stream(stream),
                       n_hist ? static_cast<const unsigned short*>(hist) : nullptr, hist_ld, hist_off, n_hist, n_new ? src : nullptr, src_ld,
                       src_off, n_new, static_cast<unsigned short*>(dst), dst_ld, static_cast<int>(rows));
    return launch_status("nbasr_stream_window_bf16");
}
