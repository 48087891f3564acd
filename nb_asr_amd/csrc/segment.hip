// Speech segmentation over CTC logits (nb_asr_amd.ctc segment / SegmentStream): the definition of include/nbasr.h "segmentation" and
// DESIGN.md 9 "Segments".  The speech decision of a frame is the endpointer's; on top of it runs an automaton with hysteresis that
// re-arms: a run of min_speech speech frames opens a segment, a run of min_silence other frames closes it (at the run's first frame),
// and a segment that reaches max_frames is closed by force.  A row carries five integers (frames, the two runs, the open segment's
// start, the segments closed so far) and a ring of its last S closed segments.  Everything after the one float compare is integer
// arithmetic, so whole = chunked = a row alone, to the bit.
//
// One wave64 per utterance, several waves per workgroup, the passes of 64 frames of endpoint.hip:
//   - speech_pass (speech_frames.h, shared with endpoint.hip) copies the pass's 64 x C floats into the wave's LDS slab and decides each
//     lane's frame; __ballot of the decision gives the pass's 64-bit mask m;
//   - the automaton walks m bit by bit.  Its state is the same in every lane of the wave (the row's index and length are made scalar
//     with readfirstlane), so a frame costs a handful of scalar instructions; lane 0 writes a closing segment's ring entry;
//   - before the first pass the wave carries the ring across: a peek (state_in != state_out) copies it, a fresh row fills it with
//     (-1, -1, -1, 0).  Those stores come from other lanes than lane 0's later ones to the same words: the first pass's barrier, a
//     workgroup-scope fence, lies between them;
//   - the row's eight head words are written once, at the end, with ordinary stores.
// Every wave of a workgroup runs the same number of passes (those of the launch's `frames`), so the two barriers of a pass are uniform;
// lanes beyond a row's length load nothing -- the columns there may hold anything -- and write 0 to the mask.
#include "speech_frames.h"

namespace nbasr {
namespace {

constexpr int kHeadWords = 8;                    // frames, speech_run, silence_run, open_start, count, 0, 0, 0
constexpr int kEntryWords = 4;                   // start, end, reason, 0
constexpr int kMaxCapacity = 64;

__global__ __launch_bounds__(kSpeechMaxWaves * 64) void segment_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const int* state_in, int* state_out, int min_speech, int min_silence,
    int max_frames, int capacity, unsigned long long speech_lo, unsigned long long speech_hi, float margin,
    unsigned char* __restrict__ mask_out, int batch, int frames, int classes, int waves)
{
    extern __shared__ float lds_frames[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * waves + wave;
    const bool row = b < batch;                  // (a workgroup's last waves may have no row: they only keep the barriers)
    float* slab = lds_frames + wave * 64 * (classes | 1);
    const int words = kHeadWords + kEntryWords * capacity;
    int* out = state_out + static_cast<size_t>(row ? b : 0) * words;

    int g0 = 0, speech_run = 0, silence_run = 0, open_start = -1, count = 0;
    int len = 0;
    if (row) {
        if (state_in) {
            const int* s = state_in + static_cast<size_t>(b) * words;
            g0 = __builtin_amdgcn_readfirstlane(s[0]); speech_run = __builtin_amdgcn_readfirstlane(s[1]);
            silence_run = __builtin_amdgcn_readfirstlane(s[2]); open_start = __builtin_amdgcn_readfirstlane(s[3]);
            count = __builtin_amdgcn_readfirstlane(s[4]);
            if (state_in != state_out) {                                     // a peek: the whole record travels, the ring before any entry
                for (int i = lane; i < kEntryWords * capacity; i += 64) out[kHeadWords + i] = s[kHeadWords + i];
            }
        } else {
            for (int i = lane; i < kEntryWords * capacity; i += 64) out[kHeadWords + i] = (i & 3) == 3 ? 0 : -1;
        }
        len = __builtin_amdgcn_readfirstlane(lengths ? lengths[b] : frames);
        len = len < 0 ? 0 : (len > frames ? frames : len);                  // (lengths[b] <= frames is the caller's to keep: nothing beyond is read)
    }
    const float* xrow = x + static_cast<size_t>(row ? b : 0) * frames * classes;

    for (int f0 = 0; f0 < frames; f0 += 64) {
        const int nf = len - f0 < 0 ? 0 : (len - f0 > 64 ? 64 : len - f0);  // this pass's frames of the row
        const bool speech = speech_pass(xrow + static_cast<size_t>(f0) * classes, slab, nf, classes, speech_lo, speech_hi, margin, lane);
        const unsigned long long m = __ballot(speech);
        for (int i = 0; i < nf; ++i) {                                      // the automaton, one frame after the other, the same in every lane
            const bool s = ((m >> i) & 1ull) != 0;
            const int g = g0 + i;
            if (s) { ++speech_run; silence_run = 0; } else { ++silence_run; speech_run = 0; }
            int end = -1, reason = 0;                                       // (a segment's end is at least 1)
            if (open_start < 0) {
                if (s && speech_run >= min_speech) open_start = g - min_speech + 1;
            } else if (!s && silence_run >= min_silence) {
                end = g - silence_run + 1;
            } else if (max_frames && g + 1 - open_start >= max_frames) {
                end = g + 1; reason = 1;
                speech_run = silence_run = 0;
            }
            if (end >= 0) {
                if (lane == 0) {
                    int* entry = out + kHeadWords + kEntryWords * (static_cast<unsigned>(count) % static_cast<unsigned>(capacity));
                    entry[0] = open_start; entry[1] = end; entry[2] = reason; entry[3] = 0;
                }
                ++count;
                open_start = -1;
            }
        }
        g0 += nf;
        if (row && mask_out && f0 + lane < frames) mask_out[static_cast<size_t>(b) * frames + f0 + lane] = speech ? 1 : 0;
        __syncthreads();                                                    // the slab is free for the next pass
    }

    if (row && lane < kHeadWords) {
        const int word = lane == 0 ? g0 : lane == 1 ? speech_run : lane == 2 ? silence_run : lane == 3 ? open_start : lane == 4 ? count : 0;
        out[lane] = word;
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_ctc_segment_state_bytes(int batch, int capacity)
{
    if (batch <= 0 || capacity < 1 || capacity > kMaxCapacity) return 0;
    return static_cast<size_t>(batch) * (kHeadWords + kEntryWords * capacity) * sizeof(int);
}

extern "C" int nbasr_ctc_segment_step(const float* x, const int* lengths, const int* state_in, int* state_out, int min_speech, int min_silence,
                                      int max_frames, int capacity, long long speech_lo, long long speech_hi, float margin,
                                      unsigned char* mask_out, int batch, int frames, int classes, nbasr_stream_t stream)
{
    static const char* who = "nbasr_ctc_segment_step";
    clear_error();
    const unsigned long long lo = static_cast<unsigned long long>(speech_lo), hi = static_cast<unsigned long long>(speech_hi);
    if (const int refused = check_speech_args(who, batch, frames, classes, margin, lo, hi)) return refused;
    NBASR_REQUIRE(min_speech >= 1 && min_silence >= 1, NBASR_EINVAL, "%s: min_speech=%d and min_silence=%d must be at least 1", who, min_speech,
                  min_silence);
    NBASR_REQUIRE(max_frames == 0 || max_frames > min_speech, NBASR_EINVAL, "%s: max_frames=%d must be 0 (none) or above min_speech=%d", who,
                  max_frames, min_speech);
    NBASR_REQUIRE(capacity >= 1 && capacity <= kMaxCapacity, NBASR_EINVAL, "%s: capacity=%d must lie in [1, %d]", who, capacity, kMaxCapacity);
    NBASR_REQUIRE(state_out && (x || frames == 0 || batch == 0), NBASR_ENULL, "%s: NULL pointer (x and state_out are required)", who);
    if (batch == 0 || (frames == 0 && state_in == state_out)) return NBASR_OK;
    const int slab_bytes = speech_slab_bytes(classes), waves = speech_waves(classes);
    const int blocks = (batch + waves - 1) / waves;
    hipLaunchKernelGGL(segment_kernel, dim3(blocks), dim3(waves * 64), static_cast<size_t>(waves) * slab_bytes, as_stream(stream), x, lengths,
                       state_in, state_out, min_speech, min_silence, max_frames, capacity, lo, hi, margin, mask_out, batch, frames, classes, waves);
    return launch_status(who);
}
