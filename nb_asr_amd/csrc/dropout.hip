// Counter-based dropout for the training path (reference ops.py:22,29,40,48 and model.py:99: nn.Dropout behind every op and in front of
// the LSTM), optionally fused with the node's sum over its flagged inputs (model.py:22).  nbasr.h gives the definition: the word of an
// element is Philox4x32-10 of (its group of four frames, the call) keyed by the seed, so the mask needs no storage, backward recomputes
// it with the same arguments, and it is the same on every launch shape and on every row slice of a batch.
//   One thread per group of four frames: one 16-byte load per operand, ten Philox rounds, one 16-byte store; a row's last, partial
//   group stores its frames one dword at a time so that the pitch columns stay untouched.  Consecutive threads take consecutive groups
//   of a row; the grid is capped and strides over the rest, every index a 64-bit number.  No LDS.
#include "common.h"

namespace nbasr {
namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 8192;                                // 256 CUs x 8 workgroups x 4: the rest is strided over

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    return Words{{c0, c1, c2, c3}};
}

// y = x * (kept ? scale : 0), then the sum as skip_sum_kernel forms it over (drop(x), skip0, skip1, skip2): each product and each sum
// rounded on its own (a contracted multiply-add would differ from dropout followed by the skip-sum launches).
#pragma clang fp contract(off)
// x / y are not __restrict__: y may be x.  A thread reads all of its group before it writes any of it, and no other thread touches it.
__global__ __launch_bounds__(kThreads) void dropout_kernel(const float* x, const float* s0, const float* s1, const float* s2, float* y,
                                                           unsigned long long total, unsigned groups, int frames, int ld,
                                                           unsigned long long thr, float scale, uint32_t seed_lo, uint32_t seed_hi,
                                                           uint32_t call_lo, uint32_t call_hi, unsigned long long row0,
                                                           unsigned long long step_rows, unsigned step_groups)
{
    unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= total) return;
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kThreads;      // = step_rows * groups + step_groups
    unsigned long long row = i / groups;                             // the one division; the stride advances (row, q) by carry
    unsigned q = static_cast<unsigned>(i - row * groups);
    for (; i < total; i += stride) {
        const unsigned long long g = (row0 + row) * groups + q;
        const Words r = philox4x32_10(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), call_lo, call_hi, seed_lo, seed_hi);
        const size_t at = static_cast<size_t>(row) * ld + 4u * q;
        f32x4 v = *reinterpret_cast<const f32x4*>(x + at);           // whole 16 bytes: ld >= round_up4(frames)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * (static_cast<unsigned long long>(r.w[e]) >= thr ? scale : 0.f);
        if (s0) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(s0 + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (0.f + v[e]) + a[e];
        }
        if (s1) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(s1 + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] + a[e];
        }
        if (s2) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(s2 + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] + a[e];
        }
        const int left = frames - static_cast<int>(4u * q);          // >= 1
        if (left >= 4) {
            *reinterpret_cast<f32x4*>(y + at) = v;
        } else {
            y[at] = v[0];
            if (left > 1) y[at + 1] = v[1];
            if (left > 2) y[at + 2] = v[2];
        }
        row += step_rows;
        q += step_groups;
        if (q >= groups) { q -= groups; ++row; }
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" int nbasr_dropout(const void* x, const void* skip0, const void* skip1, const void* skip2, void* y, int rows, int frames, int ld,
                             double p, long long seed, long long call, long long row0, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(rows >= 0 && frames >= 0, NBASR_EINVAL, "nbasr_dropout: negative size (rows=%d, frames=%d)", rows, frames);
    NBASR_REQUIRE(ld >= frames && ld % 4 == 0, NBASR_EALIGN, "nbasr_dropout: ld=%d must be >= frames=%d and a multiple of 4", ld, frames);
    NBASR_REQUIRE(p >= 0.0 && p <= 1.0, NBASR_EINVAL, "nbasr_dropout: p=%g must be in [0, 1]", p);          // (false for a NaN)
    NBASR_REQUIRE(row0 >= 0, NBASR_EINVAL, "nbasr_dropout: row0=%lld must not be negative", row0);
    NBASR_REQUIRE((skip0 || !skip1) && (skip1 || !skip2), NBASR_EINVAL, "nbasr_dropout: a skip follows a NULL skip (fill skip0, skip1, skip2 in order)");
    if (rows == 0 || frames == 0) return NBASR_OK;
    NBASR_REQUIRE(x && y, NBASR_ENULL, "nbasr_dropout: x and y must be non-NULL");
    NBASR_REQUIRE(aligned16(x) && aligned16(y) && aligned16(skip0) && aligned16(skip1) && aligned16(skip2), NBASR_EALIGN,
                  "nbasr_dropout: pointers must be 16-byte aligned");
    const unsigned long long thr = static_cast<unsigned long long>(p * 4294967296.0 + 0.5);      // floor: the value is >= 0
    const float scale = p == 1.0 ? 0.f : static_cast<float>(1.0 / (1.0 - p));
    const unsigned groups = (static_cast<unsigned>(frames) + 3u) / 4u;
    const unsigned long long total = static_cast<unsigned long long>(rows) * groups;
    const unsigned long long want = (total + kThreads - 1) / kThreads;
    const unsigned blocks = static_cast<unsigned>(want < kMaxBlocks ? want : kMaxBlocks);
    const unsigned long long stride = static_cast<unsigned long long>(blocks) * kThreads;
    const unsigned long long useed = static_cast<unsigned long long>(seed), ucall = static_cast<unsigned long long>(call);
    hipLaunchKernelGGL(dropout_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), static_cast<const float*>(x),
                       static_cast<const float*>(skip0), static_cast<const float*>(skip1), static_cast<const float*>(skip2),
                       static_cast<float*>(y), total, groups, frames, ld, thr, scale, static_cast<uint32_t>(useed),
                       static_cast<uint32_t>(useed >> 32), static_cast<uint32_t>(ucall), static_cast<uint32_t>(ucall >> 32),
                       static_cast<unsigned long long>(row0), stride / groups, static_cast<unsigned>(stride % groups));
    return launch_status("nbasr_dropout");
}
