// Utterance endpointing over CTC logits (nb_asr_amd/ctc.py endpoint / EndpointStream): the definition of include/nbasr.h "endpointing" and
// DESIGN.md 9 "Endpoint".  A frame is SPEECH iff the largest value over the speech classes exceeds the largest over the others by more than
// `margin`; a row carries six integers (frames, speech frames, first / last speech frame, endpoint frame and rule) and the first frame at
// which a rule (min_speech, min_trailing, min_frames) holds latches the endpoint.  Everything after the one float compare is integer
// arithmetic, so whole = chunked = a row alone, to the bit.
//
// One wave64 per utterance, several waves per workgroup.  A wave takes its row's frames in passes of 64, one lane per frame:
//   - the pass's 64 x C floats are contiguous in memory: the wave copies them coalesced into its LDS slab with an ODD lane stride (C | 1),
//     so the 32 lanes of a ds_read_b32 group land on 32 different banks while each lane scans its own frame in ascending class order;
//   - __ballot of the speech decision gives the pass's 64-bit mask m.  With below = m & ((2 << lane) - 1), the frames up to and including
//     the lane's own: speech_frames = carried + popcount(below); last_speech = g0 + (highest set bit of below), or the carried value;
//   - each lane evaluates the rules on those values; a second __ballot and a find-first-set give the latching frame, a shuffle its rule;
//   - the row's state lives in wave-uniform registers between passes and is written once, with ordinary stores.
// Every wave of a workgroup runs the same number of passes (those of the launch's `frames`), so the two barriers of a pass are uniform;
// lanes beyond a row's length load nothing -- the columns there may hold anything -- and write 0 to the mask.
#include "common.h"

#include <cmath>

namespace nbasr {
namespace {

constexpr int kStateWords = 8;                   // frames, speech_frames, first_speech, last_speech, endpoint_frame, endpoint_rule, 0, 0
constexpr int kMaxRules = 8;
constexpr int kMaxClasses = 128;
constexpr int kMaxWaves = 4;                     // per workgroup
constexpr int kLdsBytes = 65536;                 // a workgroup's slabs: waves * 64 * (C | 1) floats fit this

__global__ __launch_bounds__(kMaxWaves * 64) void endpoint_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const int* state_in, int* state_out, const int* __restrict__ rules,
    int n_rules, unsigned long long speech_lo, unsigned long long speech_hi, float margin, unsigned char* __restrict__ mask_out, int batch,
    int frames, int classes, int waves)
{
    extern __shared__ float lds_frames[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * waves + wave;
    const bool row = b < batch;                  // (a workgroup's last waves may have no row: they only keep the barriers)
    const int stride = classes | 1;
    float* slab = lds_frames + wave * 64 * stride;

    int g0 = 0, speech_frames = 0, first_speech = -1, last_speech = -1, endpoint_frame = -1, endpoint_rule = -1;
    int len = 0;
    if (row) {
        if (state_in) {
            const int* s = state_in + static_cast<size_t>(b) * kStateWords;
            g0 = s[0]; speech_frames = s[1]; first_speech = s[2]; last_speech = s[3]; endpoint_frame = s[4]; endpoint_rule = s[5];
        }
        len = lengths ? lengths[b] : frames;
        len = len < 0 ? 0 : (len > frames ? frames : len);                  // (lengths[b] <= frames is the caller's to keep: nothing beyond is read)
    }
    const float* xrow = x + static_cast<size_t>(row ? b : 0) * frames * classes;

    for (int f0 = 0; f0 < frames; f0 += 64) {
        const int nf = len - f0 < 0 ? 0 : (len - f0 > 64 ? 64 : len - f0);  // this pass's frames of the row
        const float* src = xrow + static_cast<size_t>(f0) * classes;
        int f = lane / classes, c = lane - f * classes;                     // element i = lane + 64 k of the pass is (frame f, class c)
        const int df = 64 / classes, dc = 64 - df * classes;
        for (int i = lane; i < nf * classes; i += 64) {
            slab[f * stride + c] = src[i];
            f += df; c += dc;
            if (c >= classes) { c -= classes; ++f; }
        }
        __syncthreads();

        bool speech = false;
        if (lane < nf) {
            const float* v = slab + lane * stride;
            float ms = -INFINITY, mn = -INFINITY;                           // maxima over the speech classes and over the others
            for (int k = 0; k < classes; ++k) {
                const bool in_s = ((k < 64 ? speech_lo >> k : speech_hi >> (k - 64)) & 1ull) != 0;
                const float val = v[k];
                if (in_s) { if (val > ms) ms = val; } else { if (val > mn) mn = val; }     // (a NaN is never taken)
            }
            speech = ms > mn + margin;
        }
        const unsigned long long m = __ballot(speech);
        const unsigned long long below = m & ((2ull << lane) - 1ull);      // (lane 63: 2 << 63 wraps to 0, minus 1 = every bit)
        const int g = g0 + lane;
        const int sf = speech_frames + __popcll(below);
        const int last = below ? g0 + 63 - __clzll(static_cast<long long>(below)) : last_speech;
        const int n_seen = g + 1;
        const int trailing = last == -1 ? n_seen : g - last;
        int fired = -1;                                                     // the lowest rule that holds at this lane's frame
        if (lane < nf) {
            for (int r = n_rules - 1; r >= 0; --r) {
                if (sf >= rules[3 * r] && trailing >= rules[3 * r + 1] && n_seen >= rules[3 * r + 2]) fired = r;
            }
        }
        const unsigned long long hits = __ballot(fired >= 0);
        if (endpoint_frame == -1 && hits) {
            const int at = __ffsll(static_cast<long long>(hits)) - 1;
            endpoint_frame = g0 + at;
            endpoint_rule = __shfl(fired, at);
        }
        if (m) {
            if (first_speech == -1) first_speech = g0 + __ffsll(static_cast<long long>(m)) - 1;
            last_speech = g0 + 63 - __clzll(static_cast<long long>(m));
            speech_frames += __popcll(m);
        }
        g0 += nf;
        if (row && mask_out && f0 + lane < frames) mask_out[static_cast<size_t>(b) * frames + f0 + lane] = speech ? 1 : 0;
        __syncthreads();                                                    // the slab is free for the next pass
    }

    if (row && lane < kStateWords) {
        const int word = lane == 0 ? g0 : lane == 1 ? speech_frames : lane == 2 ? first_speech : lane == 3 ? last_speech
                       : lane == 4 ? endpoint_frame : lane == 5 ? endpoint_rule : 0;
        state_out[static_cast<size_t>(b) * kStateWords + lane] = word;
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_ctc_endpoint_state_bytes(int batch)
{
    return batch > 0 ? static_cast<size_t>(batch) * kStateWords * sizeof(int) : 0;
}

extern "C" int nbasr_ctc_endpoint_step(const float* x, const int* lengths, const int* state_in, int* state_out, const int* rules, int n_rules,
                                       long long speech_lo, long long speech_hi, float margin, unsigned char* mask_out, int batch, int frames,
                                       int classes, nbasr_stream_t stream)
{
    static const char* who = "nbasr_ctc_endpoint_step";
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0, NBASR_EINVAL, "%s: negative sizes (batch=%d, frames=%d)", who, batch, frames);
    NBASR_REQUIRE(classes >= 2 && classes <= kMaxClasses, NBASR_EINVAL, "%s: classes=%d must lie in [2, %d]", who, classes, kMaxClasses);
    NBASR_REQUIRE(n_rules >= 1 && n_rules <= kMaxRules, NBASR_EINVAL, "%s: n_rules=%d must lie in [1, %d]", who, n_rules, kMaxRules);
    NBASR_REQUIRE(margin >= 0.f, NBASR_EINVAL, "%s: margin must be a number >= 0", who);                  // (refuses NaN too)
    const unsigned long long lo = static_cast<unsigned long long>(speech_lo), hi = static_cast<unsigned long long>(speech_hi);
    const unsigned long long all_lo = classes >= 64 ? ~0ull : (1ull << classes) - 1ull;
    const unsigned long long all_hi = classes <= 64 ? 0ull : (classes == 128 ? ~0ull : (1ull << (classes - 64)) - 1ull);
    NBASR_REQUIRE((lo & ~all_lo) == 0 && (hi & ~all_hi) == 0, NBASR_EINVAL, "%s: the speech mask names classes at or above classes=%d", who,
                  classes);
    NBASR_REQUIRE(lo != 0 || hi != 0, NBASR_EINVAL, "%s: the speech set is empty", who);
    NBASR_REQUIRE(lo != all_lo || hi != all_hi, NBASR_EINVAL, "%s: the speech set is every class: no class is left for non-speech", who);
    NBASR_REQUIRE(state_out && rules && (x || frames == 0 || batch == 0), NBASR_ENULL, "%s: NULL pointer (x, state_out and rules are required)",
                  who);
    if (batch == 0 || (frames == 0 && state_in == state_out)) return NBASR_OK;
    const int slab_bytes = 64 * (classes | 1) * static_cast<int>(sizeof(float));
    int waves = kLdsBytes / slab_bytes;
    waves = waves > kMaxWaves ? kMaxWaves : waves;                       // (128 classes: 33 KB a slab, one wave a workgroup)
    const int blocks = (batch + waves - 1) / waves;
    hipLaunchKernelGGL(endpoint_kernel, dim3(blocks), dim3(waves * 64), static_cast<size_t>(waves) * slab_bytes, as_stream(stream), x, lengths,
                       state_in, state_out, rules, n_rules, lo, hi, margin, mask_out, batch, frames, classes, waves);
    return launch_status(who);
}
