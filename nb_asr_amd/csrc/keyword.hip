// Keyword spotting over CTC logits (nb_asr_amd.ctc spot_keywords / KeywordStream): the definition of include/nbasr.h "keywords" and
// DESIGN.md 9 "Keywords".  A keyword of L tokens has S = 2 L - 1 states (token, blank, token, ...: no leading or trailing blank, the start
// is free and a match ends on its last token's frame).  Per frame V'[s] = max(stay, advance, skip the blank, for s = 0 a fresh start at 0)
// + (x[z(s)] - m), m the frame's maximum; V'[S - 1] is the log-likelihood ratio of the best path that spells the keyword and ends here
// against the unconstrained best path over the same frames, and the frame that path started at travels with it.  Every step is a float32
// compare, one subtract or one add, in an order the definition fixes, so whole = chunked = a row alone = a keyword alone, to the bit.
//
// One wave64 per (utterance, keyword), lane = state (S <= 63: a keyword has at most 32 tokens); the waves of a workgroup share one
// utterance.  The launch's frames are taken in passes of 64:
//   - the pass's 64 x C floats are contiguous in memory: the workgroup copies them coalesced into one LDS slab with an ODD lane stride
//     (C | 1), once for all its waves; after the barrier the first 64 threads take one frame each and leave its maximum (ascending class
//     order, a NaN never taken) in LDS -- the odd stride puts the 32 lanes of a ds_read_b32 group on 32 banks;
//   - after the second barrier every wave walks the pass's frames in order.  Per frame: one LDS read of x[z(lane)] (frame t's row: the
//     lanes' classes differ, stride 1 within a row), a broadcast read of m, the neighbours' V and start by lane shifts of 1 and 2
//     (__shfl_up: ds_bpermute_b32, four independent ones a frame), three compares, one subtract, one add;
//   - lane S - 1 holds the frame's score and start: it keeps the hit and the best in its own registers (the other lanes' copies are never
//     stored) and, with a trace, drops both into the wave's LDS row; after the pass's last barrier the row leaves coalesced, one lane a frame.
// V and start live in registers across passes; the row of 136 words is written once at the end with ordinary vector stores.  Every wave of
// a workgroup runs the passes of the launch's `frames`, so the three barriers of a pass are uniform; a wave without a keyword (the last
// workgroup of an utterance) helps to copy and otherwise only keeps the barriers.  Nothing at or beyond a row's length is read.
#include "common.h"

#include <cmath>

namespace nbasr {
namespace {

constexpr int kStateWords = 136;                 // frames, hit (frame, start, score), best (frame, start, score), 0, V[64], start[64]
constexpr int kHeaderWords = 8;
constexpr int kMaxTokens = 32;
constexpr int kMaxKeywords = 64;
constexpr int kMaxClasses = 128;
constexpr int kMaxWaves = 8;                     // per workgroup

__global__ __launch_bounds__(kMaxWaves * 64) void keyword_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const int* __restrict__ tokens, const int* __restrict__ token_counts,
    const float* __restrict__ thresholds, int n_keywords, int blank, const int* state_in, int* state_out, float* __restrict__ scores_out,
    int* __restrict__ starts_out, int frames, int classes, int waves, int groups)
{
    extern __shared__ float lds_pass[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, threads = waves * 64;
    const int b = blockIdx.x / groups;
    const int k = (blockIdx.x - b * groups) * waves + wave;
    const bool has = k < n_keywords;             // (an utterance's last workgroup may have waves without a keyword)
    const int stride = classes | 1;
    float* slab = lds_pass;                                                  // 64 frames at `stride` floats
    float* maxima = slab + 64 * stride;                                      // 64
    float* trace_v = maxima + 64 + wave * 128;                               // this wave's 64 scores, then its 64 starts
    int* trace_s = reinterpret_cast<int*>(trace_v + 64);

    int len = lengths ? lengths[b] : frames;
    len = len < 0 ? 0 : (len > frames ? frames : len);                      // (lengths[b] <= frames is the caller's to keep: nothing beyond is read)
    const float* xrow = x + static_cast<size_t>(b) * frames * classes;
    const size_t row = static_cast<size_t>(b) * n_keywords + (has ? k : 0);

    // the keyword: S states, lane s's class z(s), whether the blank before s may be skipped
    int S = 0, z = blank;
    bool skip = false;
    float threshold = 0.f;
    if (has) {
        int L = token_counts[k];
        L = L < 1 ? 1 : (L > kMaxTokens ? kMaxTokens : L);                  // (the tables are the caller's to keep; no lane leaves its row)
        S = 2 * L - 1;
        threshold = thresholds[k];
        if (lane < S && !(lane & 1)) {
            z = tokens[k * kMaxTokens + (lane >> 1)];
            if (lane >= 2) skip = z != tokens[k * kMaxTokens + (lane >> 1) - 1];
            if (z < 0 || z >= classes) z = blank;                           // (as above: the read stays inside the frame)
        }
    }
    const bool live = lane < S;

    // the carried row: V and start per lane, the header in every lane (lane S - 1 is the one that keeps it)
    int g = 0, hit_frame = -1, hit_start = -1, best_frame = -1, best_start = -1, start = -1;
    float hit_score = -INFINITY, best_score = -INFINITY, V = -INFINITY;
    if (has && state_in) {
        const int* s = state_in + row * kStateWords;
        g = s[0]; hit_frame = s[1]; hit_start = s[2]; hit_score = __int_as_float(s[3]);
        best_frame = s[4]; best_start = s[5]; best_score = __int_as_float(s[6]);
        if (live) { V = __int_as_float(s[kHeaderWords + lane]); start = s[kHeaderWords + 64 + lane]; }
    }

    for (int f0 = 0; f0 < frames; f0 += 64) {
        const int nf = len - f0 < 0 ? 0 : (len - f0 > 64 ? 64 : len - f0);  // this pass's frames of the row
        const float* src = xrow + static_cast<size_t>(f0) * classes;
        int f = threadIdx.x / classes, c = threadIdx.x - f * classes;      // element i = thread + threads * j of the pass is (frame f, class c)
        const int df = threads / classes, dc = threads - df * classes;
        for (int i = threadIdx.x; i < nf * classes; i += threads) {
            slab[f * stride + c] = src[i];
            f += df; c += dc;
            if (c >= classes) { c -= classes; ++f; }
        }
        __syncthreads();
        if (threadIdx.x < nf) {
            const float* v = slab + threadIdx.x * stride;
            float m = -INFINITY;
            for (int j = 0; j < classes; ++j) {
                const float val = v[j];
                if (val > m) m = val;                                       // (a NaN is never taken)
            }
            maxima[threadIdx.x] = m;
        }
        __syncthreads();

        if (has) {
            for (int t = 0; t < nf; ++t) {
                const float d = slab[t * stride + z] - maxima[t];          // one subtract
                const float v1 = __shfl_up(V, 1), v2 = __shfl_up(V, 2);
                const int s1 = __shfl_up(start, 1), s2 = __shfl_up(start, 2);
                float best = -INFINITY;
                int from = -1;
                if (V > best) { best = V; from = start; }                   // stay
                if (lane >= 1 && v1 > best) { best = v1; from = s1; }       // advance
                if (skip && v2 > best) { best = v2; from = s2; }            // skip the blank between two different tokens
                if (lane == 0 && 0.f > best) { best = 0.f; from = g; }      // a fresh start at this frame
                V = live ? best + d : -INFINITY;                            // one add
                start = live ? from : -1;
                if (lane == S - 1) {
                    if (V > best_score) { best_score = V; best_frame = g; best_start = start; }
                    if (hit_frame == -1 && V >= threshold) { hit_frame = g; hit_start = start; hit_score = V; }
                    if (scores_out) { trace_v[t] = V; trace_s[t] = start; }
                }
                ++g;
            }
        }
        __syncthreads();                                                    // the slab is free for the next pass; the trace row is whole
        if (has && scores_out && f0 + lane < frames) {
            const size_t at = row * frames + f0 + lane;
            scores_out[at] = lane < nf ? trace_v[lane] : -INFINITY;
            starts_out[at] = lane < nf ? trace_s[lane] : -1;
        }
    }

    if (has) {
        int* s = state_out + row * kStateWords;
        if (lane == S - 1) {
            s[0] = g; s[1] = hit_frame; s[2] = hit_start; s[3] = __float_as_int(hit_score);
            s[4] = best_frame; s[5] = best_start; s[6] = __float_as_int(best_score); s[7] = 0;
        }
        s[kHeaderWords + lane] = __float_as_int(V);
        s[kHeaderWords + 64 + lane] = start;
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_ctc_keyword_state_bytes(int batch, int n_keywords)
{
    return batch > 0 && n_keywords > 0 ? static_cast<size_t>(batch) * n_keywords * kStateWords * sizeof(int) : 0;
}

extern "C" int nbasr_ctc_keyword_step(const float* x, const int* lengths, const int* tokens, const int* token_counts, const float* thresholds,
                                      int n_keywords, int blank, const int* state_in, int* state_out, float* scores_out, int* starts_out,
                                      int batch, int frames, int classes, nbasr_stream_t stream)
{
    static const char* who = "nbasr_ctc_keyword_step";
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0, NBASR_EINVAL, "%s: negative sizes (batch=%d, frames=%d)", who, batch, frames);
    NBASR_REQUIRE(classes >= 2 && classes <= kMaxClasses, NBASR_EINVAL, "%s: classes=%d must lie in [2, %d]", who, classes, kMaxClasses);
    NBASR_REQUIRE(n_keywords >= 1 && n_keywords <= kMaxKeywords, NBASR_EINVAL, "%s: n_keywords=%d must lie in [1, %d]", who, n_keywords,
                  kMaxKeywords);
    NBASR_REQUIRE(blank >= 0 && blank < classes, NBASR_EINVAL, "%s: blank=%d must lie in [0, %d)", who, blank, classes);
    NBASR_REQUIRE((scores_out == nullptr) == (starts_out == nullptr), NBASR_EINVAL,
                  "%s: the trace is scores_out and starts_out together: give both or neither", who);
    NBASR_REQUIRE(state_out && tokens && token_counts && thresholds && (x || frames == 0 || batch == 0), NBASR_ENULL,
                  "%s: NULL pointer (x, tokens, token_counts, thresholds and state_out are required)", who);
    if (batch == 0 || (frames == 0 && state_in == state_out)) return NBASR_OK;
    const int waves = n_keywords > kMaxWaves ? kMaxWaves : n_keywords;
    const int groups = (n_keywords + waves - 1) / waves;
    const size_t lds_bytes = (static_cast<size_t>(64) * (classes | 1) + 64 + static_cast<size_t>(waves) * 128) * sizeof(float);
    NBASR_REQUIRE(static_cast<long long>(batch) * groups <= 0x7fffffffLL, NBASR_EINVAL, "%s: batch=%d is too large", who, batch);
    hipLaunchKernelGGL(keyword_kernel, dim3(static_cast<unsigned>(batch) * groups), dim3(waves * 64), lds_bytes, as_stream(stream), x, lengths,
                       tokens, token_counts, thresholds, n_keywords, blank, state_in, state_out, scores_out, starts_out, frames, classes, waves,
                       groups);
    return launch_status(who);
}
