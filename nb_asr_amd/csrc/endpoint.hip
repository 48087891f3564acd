// Utterance endpointing over CTC logits (nb_asr_amd.ctc endpoint / EndpointStream): the definition of include/nbasr.h "endpointing" and
// DESIGN.md 9 "Endpoint".  A frame is SPEECH iff the largest value over the speech classes exceeds the largest over the others by more than
// `margin`; a row carries six integers (frames, speech frames, first / last speech frame, endpoint frame and rule) and the first frame at
// which a rule (min_speech, min_trailing, min_frames) holds latches the endpoint.  Everything after the one float compare is integer
// arithmetic, so whole = chunked = a row alone, to the bit.
//
// One wave64 per utterance, several waves per workgroup.  A wave takes its row's frames in passes of 64, one lane per frame:
//   - speech_pass (speech_frames.h, shared with segment.hip) copies the pass's 64 x C floats into the wave's LDS slab and decides each
//     lane's frame;
//   - __ballot of the speech decision gives the pass's 64-bit mask m.  With below = m & ((2 << lane) - 1), the frames up to and including
//     the lane's own: speech_frames = carried + popcount(below); last_speech = g0 + (highest set bit of below), or the carried value;
//   - each lane evaluates the rules on those values; a second __ballot and a find-first-set give the latching frame, a shuffle its rule;
//   - the row's state lives in wave-uniform registers between passes and is written once, with ordinary stores.
// Every wave of a workgroup runs the same number of passes (those of the launch's `frames`), so the two barriers of a pass are uniform;
// lanes beyond a row's length load nothing -- the columns there may hold anything -- and write 0 to the mask.
#include "speech_frames.h"

namespace nbasr {
namespace {

constexpr int kStateWords = 8;                   // frames, speech_frames, first_speech, last_speech, endpoint_frame, endpoint_rule, 0, 0
constexpr int kMaxRules = 8;

__global__ __launch_bounds__(kSpeechMaxWaves * 64) void endpoint_kernel(
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
        const bool speech = speech_pass(xrow + static_cast<size_t>(f0) * classes, slab, nf, classes, speech_lo, speech_hi, margin, lane);
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
    const unsigned long long lo = static_cast<unsigned long long>(speech_lo), hi = static_cast<unsigned long long>(speech_hi);
    if (const int refused = check_speech_args(who, batch, frames, classes, margin, lo, hi)) return refused;
    NBASR_REQUIRE(n_rules >= 1 && n_rules <= kMaxRules, NBASR_EINVAL, "%s: n_rules=%d must lie in [1, %d]", who, n_rules, kMaxRules);
    NBASR_REQUIRE(state_out && rules && (x || frames == 0 || batch == 0), NBASR_ENULL, "%s: NULL pointer (x, state_out and rules are required)",
                  who);
    if (batch == 0 || (frames == 0 && state_in == state_out)) return NBASR_OK;
    const int slab_bytes = speech_slab_bytes(classes), waves = speech_waves(classes);
    const int blocks = (batch + waves - 1) / waves;
    hipLaunchKernelGGL(endpoint_kernel, dim3(blocks), dim3(waves * 64), static_cast<size_t>(waves) * slab_bytes, as_stream(stream), x, lengths,
                       state_in, state_out, rules, n_rules, lo, hi, margin, mask_out, batch, frames, classes, waves);
    return launch_status(who);
}
