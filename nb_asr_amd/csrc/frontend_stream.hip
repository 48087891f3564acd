// Incremental feature front-end (nb_asr_amd/frontend.py FrontendStream): the chain of frontend.hip -- centred reflect-padded frames,
// windowed DFT, power, mel filterbank, log, normalisation -- as ONE launch per push of a waveform stream, with no intermediate in
// device memory.  The host decides which frames a push makes final (frontend.py: frames_final / frames_total / retain_from); the
// kernel reflects sample indices and nothing else.
//
// A workgroup of 13 waves owns 16 consecutive frames of one utterance:
//   1. gather the 16 x 400 samples of its frames into LDS, frames[k][t] (source: the retained tail or this push's samples, by
//      absolute sample index);
//   2. DFT on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32): wave w computes bins 16 w .. 16 w + 15 of all 16 frames, the
//      cosine and the sine rows in two accumulators, so re^2 + im^2 is formed in registers; power (208, 16) goes to LDS
//      (rows 201..207 come out zero: the matrix rows are zero there);
//   3. waves 0..4: mel filterbank (80 x 208) as a second GEMM on the same instruction, then log, shift, scale, store in the
//      model's input layout.
// Both GEMMs run k in ascending order in one accumulator chain per output, so a frame's features are a function of its 400 samples
// alone: the same bits whatever the push sizes, the frame's place in a tile or the batch.
// One more workgroup per utterance copies the samples the next push still needs into the OTHER tail buffer.
//
// The matrices arrive as operand images in the order the lanes read them (16 bytes per lane, 1 KB per wave and k block):
//   dft image   [13 bin tiles][cos | sin][25 k blocks][64 lanes][4]: lane l, element s = row 16 tile + (l & 15), k = 16 kb + 4 s + (l >> 4)
//   fbank image [5 mel tiles][13 k blocks][64 lanes][4]            : the same map over the (80, 208) filterbank
#include "sample_tail.h"

namespace nbasr {
namespace {

constexpr int kWin = 400, kHop = 160, kBins = 201, kBinsPad = 208, kMels = 80;
constexpr int kTile = 16;                        // frames per workgroup
constexpr int kBinTiles = kBinsPad / 16, kMelTiles = kMels / 16, kDftBlocks = kWin / 16, kMelBlocks = kBinsPad / 16;
constexpr int kThreads = 64 * kBinTiles;         // 832: one wave per bin tile
constexpr int kFrameLd = 17;                     // LDS pitch of frames[k][.]: the gather's writes (k along the lanes) spread over the banks
constexpr int kTailLd = (kWin + 1 + 3) / 4 * 4;  // 404 floats per utterance and tail

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads) void frontend_stream_kernel(
    const float* __restrict__ tail_in, int tail_len, long long tail_first, const float* __restrict__ wave, int n_new, int ld_wave,
    float* __restrict__ tail_out, int tail_out_first_rel, const float4* __restrict__ dft, const float4* __restrict__ fbank,
    const float* __restrict__ mean, const float* __restrict__ inv_scale, float* __restrict__ feats, int ld_feats, int col0,
    int first_frame, int n_frames, long long total_len, int final, int n_tiles)
{
    __shared__ float frames[kWin * kFrameLd];
    __shared__ float power[kBinsPad * kTile];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const Samples src{tail_in + static_cast<size_t>(b) * kTailLd, wave + static_cast<size_t>(b) * ld_wave, tail_first, tail_len, n_new};

    if (tile == n_tiles) {                       // the trailing workgroup: what the next push still needs
        const int out_len = tail_len + n_new - tail_out_first_rel;
        float4* __restrict__ dst = reinterpret_cast<float4*>(tail_out + static_cast<size_t>(b) * kTailLd);
        for (int q = tid; q < kTailLd / 4; q += kThreads) {
            float v[4];
            for (int c = 0; c < 4; ++c) v[c] = 4 * q + c < out_len ? src.at(tail_first + tail_out_first_rel + 4 * q + c) : 0.f;
            dst[q] = make_float4(v[0], v[1], v[2], v[3]);
        }
        return;
    }

    const int t0 = tile * kTile;
    for (int idx = tid; idx < kTile * kWin; idx += kThreads) {
        const int t = idx / kWin, k = idx - t * kWin;
        float v = 0.f;
        if (t0 + t < n_frames) {
            long long i = static_cast<long long>(first_frame + t0 + t) * kHop + k - kWin / 2;
            if (i < 0) i = -i;
            if (final && i >= total_len) i = 2 * (total_len - 1) - i;
            v = src.at(i);
        }
        frames[k * kFrameLd + t] = v;
    }
    __syncthreads();

    const int w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    {
        const float4* __restrict__ a_cos = dft + static_cast<size_t>(w) * 2 * kDftBlocks * 64 + lane;
        const float4* __restrict__ a_sin = a_cos + kDftBlocks * 64;
        f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
        for (int kb = 0; kb < kDftBlocks; ++kb) {
            const float4 c = a_cos[kb * 64], s = a_sin[kb * 64];
            const float* __restrict__ fr = frames + (kb * 16 + kq) * kFrameLd + col;
            const float x0 = fr[0], x1 = fr[4 * kFrameLd], x2 = fr[8 * kFrameLd], x3 = fr[12 * kFrameLd];
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(c.x, x0, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(s.x, x0, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(c.y, x1, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(s.y, x1, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(c.z, x2, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(s.z, x2, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(c.w, x3, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(s.w, x3, im, 0, 0, 0);
        }
        for (int r = 0; r < 4; ++r)              // accumulator r of lane (col, kq) = bin 16 w + 4 kq + r of frame col
            power[(w * 16 + kq * 4 + r) * kTile + col] = __builtin_fmaf(re[r], re[r], im[r] * im[r]);
    }
    __syncthreads();
    if (w >= kMelTiles) return;

    const float4* __restrict__ a_fb = fbank + static_cast<size_t>(w) * kMelBlocks * 64 + lane;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < kMelBlocks; ++kb) {
        const float4 a = a_fb[kb * 64];
        const float* __restrict__ pw = power + (kb * 16 + kq) * kTile + col;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, pw[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, pw[4 * kTile], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, pw[8 * kTile], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, pw[12 * kTile], acc, 0, 0, 0);
    }
    if (t0 + col < n_frames) {
        for (int r = 0; r < 4; ++r) {
            const int m = w * 16 + kq * 4 + r;
            feats[(static_cast<size_t>(b) * kMels + m) * ld_feats + col0 + t0 + col] = (logf(acc[r]) - mean[m]) * inv_scale[m];
        }
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_frontend_stream_state_bytes(int batch, int win)
{
    if (batch <= 0 || win <= 0) return 0;
    return static_cast<size_t>(2) * batch * ((win + 1 + 3) / 4 * 4) * sizeof(float);
}

extern "C" int nbasr_frontend_stream_step(const float* tail_in, int tail_len, long long tail_first, const float* wave, int n_new, int ld_wave,
                                          float* tail_out, int tail_out_first_rel, const float* dft, const float* fbank, const float* mean,
                                          const float* inv_scale, float* feats, int ld_feats, int col0, int first_frame, int n_frames,
                                          long long total_len, int final, int batch, int win, int hop, int bins, int n_mels,
                                          nbasr_stream_t stream)
{
    static const char* who = "nbasr_frontend_stream_step";
    clear_error();
    NBASR_REQUIRE(win == kWin && hop == kHop && bins == kBins && n_mels == kMels, NBASR_EINVAL,
                  "nbasr_frontend_stream_step: unsupported geometry win=%d hop=%d bins=%d n_mels=%d (built for %d / %d / %d / %d)", win, hop, bins,
                  n_mels, kWin, kHop, kBins, kMels);
    if (const int rc = tail_step_sizes(who, kTailLd, batch, tail_len, tail_first, n_new, ld_wave, first_frame >= 0 && n_frames >= 0 && col0 >= 0,
                                       total_len)) return rc;
    NBASR_REQUIRE(!final || total_len > win / 2, NBASR_EINVAL, "nbasr_frontend_stream_step: reflect padding needs more than %d samples", win / 2);
    const bool retain = !final && tail_out != nullptr;      // (tail_out == NULL: a step that emits some frames of a push and leaves the tail alone)
    if (batch == 0 || (n_frames == 0 && (n_new == 0 || !retain))) return NBASR_OK;
    if (const int rc = tail_step_pointers(who, batch, tail_in, tail_len, wave, n_new)) return rc;
    if (n_frames > 0) {
        NBASR_REQUIRE(dft && fbank && mean && inv_scale && feats, NBASR_ENULL, "nbasr_frontend_stream_step: NULL pointer");
        NBASR_REQUIRE(ld_feats % 4 == 0 && aligned16(dft) && aligned16(fbank), NBASR_EALIGN,
                      "nbasr_frontend_stream_step: ld_feats=%d must be a multiple of 4, the matrix images 16-byte aligned", ld_feats);
        NBASR_REQUIRE(col0 + static_cast<long long>(n_frames) <= ld_feats, NBASR_EINVAL,
                      "nbasr_frontend_stream_step: columns %d..%lld do not fit ld_feats=%d", col0, col0 + static_cast<long long>(n_frames) - 1, ld_feats);
        // every sample the frames touch, reflection applied, must be in [tail_first, total_len)
        const long long first_lo = static_cast<long long>(first_frame) * hop - win / 2;
        const long long hi = (static_cast<long long>(first_frame) + n_frames - 1) * hop + win / 2 - 1;
        long long lo = first_lo < 0 ? 0 : first_lo, top = hi;
        if (first_lo < 0 && -first_lo > top) top = -first_lo;
        if (final && top >= total_len) {
            const long long back = 2 * (total_len - 1) - top;
            if (back < lo) lo = back;
            top = total_len - 1;
        }
        NBASR_REQUIRE(lo >= tail_first && top < total_len, NBASR_EINVAL,
                      "nbasr_frontend_stream_step: frames %d..%lld need samples %lld..%lld, the stream holds %lld..%lld", first_frame,
                      static_cast<long long>(first_frame) + n_frames - 1, lo, top, tail_first, total_len - 1);
    }
    if (retain)
        if (const int rc = tail_step_retain(who, kTailLd, tail_in, tail_len, n_new, tail_out, tail_out_first_rel)) return rc;
    const int n_tiles = (n_frames + kTile - 1) / kTile;
    hipLaunchKernelGGL(frontend_stream_kernel, dim3(n_tiles + (retain ? 1 : 0), batch), dim3(kThreads), 0, as_stream(stream), tail_in, tail_len,
                       tail_first, wave, n_new, ld_wave, tail_out, tail_out_first_rel, reinterpret_cast<const float4*>(dft),
                       reinterpret_cast<const float4*>(fbank), mean, inv_scale, feats, ld_feats, col0, first_frame, n_frames, total_len, final,
                       n_tiles);
    return launch_status(who);
}
